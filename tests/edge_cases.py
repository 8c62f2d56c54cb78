"""Small operators that sit exactly on the data-dependent limits of the storage formats, and
oracle-independent references for them (plain numpy / scipy: no GPU, no oracle).

Exact integers.  Every zoo matrix has integer-valued entries with |a| <= 2^11, and int_vectors
gives integer-valued x (|x| <= 2^10, no zeros), y0 and b (|b| <= 2^40).  While sum |a||x| + |b|
stays below 2^53 for every row (assert_exact_range), every partial sum of every summation
order is an integer below 2^53: fp64 arithmetic is exact in any order, and the expected result
is an int64 product -- compared bit for bit (bits), independently of the CPU oracle.  With a
power-of-two diagonal and omega = 0.5 the Jacobi update is exact as well: (b - Ax) / (2 a_ii)
is an integer of < 2^42 over 2^12.

Fixed points.  With b = A x formed in int64 every residual is exactly +0.0, so jacobi, hybrid_gs
and hybrid_gs_backward return x bit for bit whatever the (l1) diagonal and block size.

Poisoned columns.  With x[c] = inf or nan, a row that stores no entry in column c must give
the bits it gives with a finite x[c]: a padding entry, a padded tile line or a masked
template slot leaking into a row sum would turn it into nan.

The cut rule (build_row_blocks, raptor_amd/csrc/par_matrix.hip), restated by cut_blocks:
rows are taken greedily; a block is closed before row r (r > its first row) when
  * its entries plus row r's exceed kCAP = 2048, or
  * it already holds 256 rows, or
  * its distinct x lines plus row r's new ones exceed 2048 / lw (lw = 8 doubles: 256 lines of
    64 B; lw = 4: 512 lines of 32 B), or
  * row r's "handled by a row template" flag differs from the block's.
A single row over one of the caps is a block of its own."""
import functools
from dataclasses import dataclass, field

import numpy as np
import scipy.sparse as sp

CAP = 2048          # kCAP: nonzeros per row block
ROWS = 256          # kTPB: rows per row block
TPL_MAX = 255       # kTplMax
TPL_ENTRIES = 1024  # kTplEntries
TPL_MAX_LEN = 64    # kTplMaxLen
GS_WIDE = 128       # kGsWide
POW2 = 2 ** np.arange(12)  # the diagonal values: 1 .. 2048


def bits(a):
    """The bit patterns of a float64 array: +0.0 != -0.0, and a nan equals itself."""
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


# ---- exact references (int64) -------------------------------------------------------------
def _int(v):
    v = np.asarray(v, np.float64)
    iv = v.astype(np.int64)
    assert np.array_equal(iv.astype(np.float64), v), "not integer-valued"
    return iv


def _imat(A):
    A = A.tocsr()
    return sp.csr_matrix((_int(A.data), A.indices, A.indptr), shape=A.shape)


def assert_exact_range(A, x, b=None, y0=None):
    """Every row's sum |a_ij||x_j| (+ |b_i|, + |y0_i|) stays below 2^53, in int64."""
    M = _imat(A)
    M.data = np.abs(M.data)
    s = M @ np.abs(_int(x))
    for v in (b, y0):
        if v is not None:
            s = s + np.abs(_int(v))
    # int64 itself cannot overflow here: <= 2^13 entries per row * 2^11 * 2^10, + 2^40
    assert A.shape[1] <= 1 << 20 and np.abs(M.data).max(initial=0) <= 1 << 11
    assert s.max(initial=0) < 1 << 53, "partial sums could round"
    return True


def exact_spmv(A, x):
    assert_exact_range(A, x)
    return (_imat(A) @ _int(x)).astype(np.float64)


def exact_spmv_add(A, x, y0):
    assert_exact_range(A, x, y0=y0)
    return (_int(y0) + _imat(A) @ _int(x)).astype(np.float64)


def exact_residual(A, x, b):
    assert_exact_range(A, x, b)
    return (_int(b) - _imat(A) @ _int(x)).astype(np.float64)


def exact_residual_norm(A, x, b):
    """sqrt of the exact sum of squares (Python integers: no overflow, one rounding each in
    the conversion and the square root)."""
    assert_exact_range(A, x, b)
    r = _int(b) - _imat(A) @ _int(x)
    return float(np.sqrt(np.float64(sum(int(v) * int(v) for v in r))))


def exact_jacobi(A, x, b, omega=0.5):
    """x + (b - A x) / (2 a_ii) for power-of-two a_ii: numerator in int64, one exact scaling."""
    assert omega == 0.5
    assert_exact_range(A, x, b)
    d = _int(A.diagonal())
    assert np.all(d > 0) and np.all(d & (d - 1) == 0), "diagonal must be a positive power of two"
    r = _int(b) - _imat(A) @ _int(x)
    num = _int(x) * (2 * d) + r  # |.| < 2^10 * 2^12 + 2^41
    assert np.abs(num).max(initial=0) < 1 << 53
    return num.astype(np.float64) / (2 * d).astype(np.float64)  # exact: a power-of-two divisor


def b_for_fixed_point(A, x):
    assert_exact_range(A, x)
    b = _imat(A) @ _int(x)
    assert np.abs(b).max(initial=0) < 1 << 52  # |b| + sum |a||x| < 2^53
    return b.astype(np.float64)


def exact_matmat(A, B, pattern=None):
    """int64 values of A @ B on `pattern` (CSR; default: the structural product's own).  The
    structural pattern keeps entries whose value cancels to zero."""
    Ai, Bi = _imat(A), _imat(B)
    amax = int(np.abs(Ai.data).max(initial=0)) * int(np.abs(Bi.data).max(initial=0))
    assert amax * max(1, int(np.diff(Ai.indptr).max(initial=0))) < 1 << 53
    C = (Ai @ Bi).tocsr()
    C.sort_indices()
    if pattern is None:
        return C
    P = pattern.tocsr()
    out = np.empty(P.nnz, np.int64)
    for i in range(P.shape[0]):
        row = dict(zip(C.indices[C.indptr[i]:C.indptr[i + 1]].tolist(),
                       C.data[C.indptr[i]:C.indptr[i + 1]].tolist()))
        for k in range(P.indptr[i], P.indptr[i + 1]):
            out[k] = row.get(int(P.indices[k]), 0)
    return sp.csr_matrix((out, P.indices, P.indptr), shape=P.shape)


def structural_product(A, B):
    """The pattern of A @ B with every structural entry kept (values 1)."""
    Ap = sp.csr_matrix((np.ones(A.nnz, np.int64), A.indices, A.indptr), shape=A.shape)
    Bp = sp.csr_matrix((np.ones(B.nnz, np.int64), B.indices, B.indptr), shape=B.shape)
    C = (Ap @ Bp).tocsr()
    C.sort_indices()
    return C


def int_vectors(n, seed):
    """(x, y0, b): integer-valued; 1 <= |x| <= 2^10, |y0| <= 2^10, |b| <= 2^40."""
    rng = np.random.default_rng(seed)
    x = rng.integers(1, (1 << 10) + 1, n) * rng.choice([-1, 1], n)
    y0 = rng.integers(-(1 << 10), (1 << 10) + 1, n)
    b = rng.integers(-(1 << 40), (1 << 40) + 1, n)
    return x.astype(np.float64), y0.astype(np.float64), b.astype(np.float64)


def rows_without(A, c):
    """Mask of the rows that store no entry in column c."""
    A = A.tocsr()
    hit = np.zeros(A.shape[0], bool)
    rows = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
    hit[rows[A.indices == c]] = True
    return ~hit


def poison_columns(A, blocks=None):
    """Columns 0, n - 1, one in the middle of a row block and one at a block's first row."""
    n = A.shape[0]
    blocks = blocks or cut_blocks(A)
    q = blocks[len(blocks) // 2]
    return sorted({0, n - 1, min(n - 1, (q[0] + q[1]) // 2), q[0]})


# ---- the builders' rules, restated ----------------------------------------------------------
def cut_blocks(A, lw=8, tplf=None):
    """build_row_blocks' greedy cut (one rank, one chunk: every zoo case is below 4096 rows or
    2^20 nonzeros): the list of [r0, r1)."""
    A = A.tocsr()
    n, rp, col = A.shape[0], A.indptr, A.indices
    cap_lines = CAP // lw
    out, r0, acc, lines = [], 0, 0, set()
    for r in range(n):
        mine = set((col[rp[r]:rp[r + 1]] // lw).tolist())
        ln = int(rp[r + 1] - rp[r])
        if r > r0 and (acc + ln > CAP or r - r0 >= ROWS or len(lines | mine) > cap_lines or
                       (tplf is not None and tplf[r] != tplf[r0])):
            out.append((r0, r))
            r0, acc, lines = r, 0, set()
        lines |= mine
        acc += ln
    if n > r0:
        out.append((r0, n))
    return out


def block_lines(A, blk, lw=8):
    A = A.tocsr()
    return len(set((A.indices[A.indptr[blk[0]]:A.indptr[blk[1]]] // lw).tolist()))


def block_values(A, blk):
    """Distinct bit patterns among a block's stored values."""
    A = A.tocsr()
    return len(np.unique(bits(A.data[A.indptr[blk[0]]:A.indptr[blk[1]]])))


def vi_blocks(A, blocks):
    """Blocks the value index takes: 1 .. kCAP entries of <= 256 distinct bit patterns."""
    A = A.tocsr()
    nz = [int(A.indptr[b[1]] - A.indptr[b[0]]) for b in blocks]
    return sum(1 for b, z in zip(blocks, nz) if 0 < z <= CAP and block_values(A, b) <= 256)


def row_templates(A, min_rows=16384):
    """build_templates + the rule that takes them: (per-row flag or None, templates, rows).
    A row qualifies with 1 .. 64 entries; rows with equal (column - row, value bits) and equal
    1 / a_ii share a template; templates are taken in order of first appearance while there
    are fewer than 255 and their entries, each run padded to a multiple of 4, stay <= 1024.
    They are used when they cover every row, or at least half the rows of an operator of
    >= min_rows (AMG_TPL_MIN_ROWS) rows."""
    A = A.tocsr()
    n, rp, col, val = A.shape[0], A.indptr, A.indices, A.data
    d = A.diagonal()
    seen, ent, flag = {}, 0, np.zeros(n, np.uint8)
    for r in range(n):
        ln = int(rp[r + 1] - rp[r])
        if ln < 1 or ln > TPL_MAX_LEN:
            continue
        with np.errstate(divide="ignore"):
            dinv = np.float64(1.0) / np.float64(d[r])
        key = ((col[rp[r]:rp[r + 1]] - r).tobytes(), bits(val[rp[r]:rp[r + 1]]).tobytes(),
               bits(np.array([dinv])).tobytes())
        if key not in seen:
            pad = (ln + 3) & ~3
            ok = sum(seen.values()) < TPL_MAX and ent + pad <= TPL_ENTRIES
            seen[key] = ok
            ent += pad if ok else 0
        flag[r] = seen[key]
    rows, ntpl = int(flag.sum()), sum(seen.values())
    if n and (rows == n or (n >= min_rows and 2 * rows >= n)):
        return flag, ntpl, rows
    return None, 0, 0


def chain_widths(A, B=64):
    """(forward, backward): the most stored couplings of any row to rows before / after it
    inside its chunk of B rows (the split sweep's chain-walk queue depth)."""
    A = A.tocsr()
    n = A.shape[0]
    rows = np.repeat(np.arange(n), np.diff(A.indptr))
    same = rows // B == A.indices // B
    fw = np.bincount(rows[same & (A.indices < rows)], minlength=n)
    bw = np.bincount(rows[same & (A.indices > rows)], minlength=n)
    return int(fw.max(initial=0)), int(bw.max(initial=0))


def ell_slabs(A, B=64):
    """(slabs, cells) of the sliced-ELL sweep without GS templates: whole chunks of B rows
    packed into slabs of <= 64 rows, each as wide as its longest row rounded up to 4."""
    A = A.tocsr()
    n, ln = A.shape[0], np.diff(A.indptr)
    r, slabs, cells = 0, 0, 0
    while r < n:
        end = r
        while end < n:
            ce = min(n, (end // B + 1) * B)
            if ce - r > 64:
                break
            end = ce
        slabs += 1
        cells += (int(ln[r:end].max()) + 3) & ~3
        r = end
    return slabs, cells


# ---- the zoo ---------------------------------------------------------------------------------
@dataclass
class Case:
    name: str
    group: str
    A: sp.csr_matrix
    n_blocks: int                 # hand-derived (the builder's docstring), under set_format("blocks")
    doc: str = ""
    env: dict = field(default_factory=dict)  # AMG_* knobs set before from_csr
    lw: int = 8                   # x-tile line width the derivation assumes
    full_diag: bool = True        # every row stores a positive power-of-two diagonal
    n_vi_blocks: int = None
    n_templates: int = None       # format auto
    template_rows: int = None     # format auto
    tile_line_bytes: int = None
    gs_width: int = None          # widest in-chunk coupling at B = 64, both directions
    ell_wide: bool = False        # sliced-ELL sweep on its wide variant
    n_values: int = None          # distinct bit patterns of the whole operator (GS dictionary)


_BUILDERS = []


def _case(group, **kw):
    def deco(fn):
        _BUILDERS.append((fn.__name__, group, fn, kw))
        return fn
    return deco


def _values(rng, nnz):
    v = rng.integers(1, (1 << 11) + 1, nnz) * rng.choice([-1, 1], nnz)
    return v.astype(np.float64)


def _assemble(n, rows, rng=None, vals=None):
    """CSR from per-row sorted column arrays.  Values: `vals` (per-row arrays) or random
    integers in [-2^11, 2^11] \\ {0}; a stored diagonal gets a random power of two unless vals
    is given."""
    rp = np.zeros(n + 1, np.int64)
    rp[1:] = np.cumsum([len(c) for c in rows])
    col = np.concatenate([np.asarray(c, np.int64) for c in rows]) if rp[-1] else np.zeros(0, np.int64)
    if vals is not None:
        val = np.concatenate([np.asarray(v, np.float64) for v in vals]) if rp[-1] else np.zeros(0)
    else:
        val = _values(rng, int(rp[-1]))
        r = np.repeat(np.arange(n), np.diff(rp))
        dg = col == r
        val[dg] = rng.choice(POW2, int(dg.sum())).astype(np.float64)
    assert all(np.all(np.diff(c) > 0) for c in rows if len(c) > 1), "columns must ascend"
    return sp.csr_matrix((val, col.astype(np.int32), rp.astype(np.int32)), shape=(n, n))


def _window(i, n, w, before):
    """w consecutive columns containing i: from i - before, clamped to [0, n - w]."""
    s = min(max(i - before, 0), n - w)
    return np.arange(s, s + w)


@_case("cap_nnz")
def cap_nnz_exact():
    """512 rows of exactly 8 entries.  Rows 0..255 hold 256 * 8 = 2048 = kCAP entries: row 256
    does not fit (and is the 257th row).  2 blocks of exactly kCAP entries."""
    n = 512
    return _assemble(n, [_window(i, n, 8, 3) for i in range(n)], np.random.default_rng(101)), 2


@_case("cap_nnz")
def cap_nnz_plus1():
    """cap_nnz_exact with 9 entries in row 100.  Rows 0..254 hold 254 * 8 + 9 = 2041 entries and
    row 255 would make 2049 > kCAP: block [0, 255).  Rows 255..510 are 256 rows of 2048
    entries: block [255, 511) (full in rows and entries).  Row 511 alone.  3 blocks."""
    n = 512
    rows = [_window(i, n, 9 if i == 100 else 8, 3) for i in range(n)]
    return _assemble(n, rows, np.random.default_rng(102)), 3


@_case("cap_nnz")
def cap_nnz_long_rows():
    """Rows of 2047 (row 0, the first), 2048 (row 1000), 2049 (row 2000), 4096 (row 3000) and
    4097 (row 4199, the last) consecutive columns; every other row stores its diagonal only.
    n = 4200.
      [0, 2): 2047 + 1 = 2048 entries on lines 0..255 (exactly a tile); row 2 would be 2049.
      rows 2..999 (998 one-entry rows): 256 + 256 + 256 + 230 -> 4 blocks.
      row 1000 (2048 entries, 256 lines): alone, the x-tile path with a full stage.
      rows 1001..1999 (999 rows): 3 * 256 + 231 -> 4 blocks.
      row 2000 (2049 entries): alone, the long path: one full chunk + 1 entry.
      rows 2001..2999: 4 blocks.
      row 3000 (4096 entries): alone, two exactly full chunks.
      rows 3001..4198 (1198 rows): 4 * 256 + 174 -> 5 blocks.
      row 4199 (4097 entries): alone, two chunks + 1 entry.
    1 + 4 + 1 + 4 + 1 + 4 + 1 + 5 + 1 = 22 blocks."""
    n = 4200
    rows = [np.array([i]) for i in range(n)]
    rows[0] = np.arange(0, 2047)
    rows[1000] = np.arange(0, 2048)
    rows[2000] = np.arange(0, 2049)
    rows[3000] = np.arange(0, 4096)
    rows[4199] = np.arange(n - 4097, n)
    return _assemble(n, rows, np.random.default_rng(103)), 22


def _diag_rows(n, keep, seed):
    rows = [np.array([i]) if keep[i] else np.zeros(0, np.int64) for i in range(n)]
    return _assemble(n, rows, np.random.default_rng(seed))


@_case("cap_rows")
def cap_rows_255():
    """255 rows of one entry: 1 block, one row short of the row cap."""
    return _diag_rows(255, np.ones(255, bool), 111), 1


@_case("cap_rows")
def cap_rows_256():
    """256 rows of one entry: exactly the row cap (kTPB), 1 block."""
    return _diag_rows(256, np.ones(256, bool), 112), 1


@_case("cap_rows")
def cap_rows_257():
    """257 rows of one entry: [0, 256) and a block of one row.  2 blocks."""
    return _diag_rows(257, np.ones(257, bool), 113), 2


@_case("cap_rows")
def cap_rows_513():
    """513 rows of one entry: 256 + 256 + 1.  3 blocks."""
    return _diag_rows(513, np.ones(513, bool), 114), 3


@_case("cap_rows", full_diag=False)
def cap_rows_gaps():
    """1100 rows of one (diagonal) entry, with rows 250..799 and 1000..1009 empty.  Nothing
    but the row cap cuts: [0, 256), [256, 512), [512, 768), [768, 1024), [1024, 1100):
    5 blocks.  [256, 512) and [512, 768) hold empty rows only (the empty-block path); the
    others mix empty and one-entry rows."""
    n = 1100
    keep = np.ones(n, bool)
    keep[250:800] = False
    keep[1000:1010] = False
    return _diag_rows(n, keep, 115), 5


@_case("cap_rows", full_diag=False)
def cap_rows_nnz0():
    """300 rows, no entry at all (nnz == 0): [0, 256), [256, 300).  2 blocks."""
    return _diag_rows(300, np.zeros(300, bool), 116), 2


def _lines_matrix(lw, extra_row, seed):
    """n = 2056.  Rows 0..7: the diagonal and 2048 / lw / 8 entries lw columns apart -- row i
    touches lines [i * L, (i + 1) * L), L = 2048 / lw / 8 -- so rows 0..7 touch exactly the
    2048 / lw lines of columns 0..2047.  Row `extra_row` also stores column 2048 (one more
    line).  Rows 9.. store their diagonal only."""
    n, L = 2056, CAP // lw // 8
    rows = []
    for i in range(n):
        c = {i}
        if i < 8:
            c |= {lw * (L * i + j) for j in range(L)}
        if i == extra_row:
            c.add(2048)
        rows.append(np.array(sorted(c)))
    return _assemble(n, rows, np.random.default_rng(seed))


@_case("cap_lines", env={"AMG_TILE_LINE": "8"}, tile_line_bytes=64)
def cap_lines_256():
    """64-byte lines, entries 8 columns apart.  Rows 0..7 touch lines 0..255: exactly the 256
    lines of a tile (their diagonals, columns 0..7, are on line 0).  Row 8 stores column 2048,
    line 256: a 257th line, so the block closes before row 8: [0, 8).  Rows 8..2055 (2048
    rows; row 8's two lines, then one diagonal each: 32 lines per 256 rows) are cut by the row
    cap alone: 8 blocks.  9 blocks."""
    return _lines_matrix(8, 8, 121), 9


@_case("cap_lines", env={"AMG_TILE_LINE": "8"}, tile_line_bytes=64)
def cap_lines_257():
    """cap_lines_256 with column 2048 stored in row 7 instead: rows 0..6 touch lines 0..223, row
    7 adds 224..255 and 256 -> 257 lines: the cut moves one row up, [0, 7).  Rows 7..2055 are
    2049 rows: 8 * 256 + 1 -> 9 blocks.  10 blocks."""
    return _lines_matrix(8, 7, 122), 10


@_case("cap_lines", env={"AMG_TILE_LINE": "4"}, lw=4, tile_line_bytes=32)
def cap_lines_512():
    """32-byte lines (AMG_TILE_LINE=4), entries 4 columns apart.  Rows 0..7 touch lines 0..511:
    exactly the 512 lines of a tile.  Row 8 stores column 2048 (line 512): [0, 8), then the
    row cap: 8 blocks.  9 blocks."""
    return _lines_matrix(4, 8, 123), 9


@_case("cap_lines", env={"AMG_TILE_LINE": "4"}, lw=4, tile_line_bytes=32)
def cap_lines_513():
    """cap_lines_512 with column 2048 in row 7: 448 + 64 + 1 = 513 lines at row 7, the cut moves
    one row up: [0, 7), then 2049 rows -> 9 blocks.  10 blocks."""
    return _lines_matrix(4, 7, 124), 10


@_case("cap_lines", env={"AMG_TILE_LINE": "8"}, tile_line_bytes=64)
def cap_lines_long_row():
    """n = 2500, one-entry (diagonal) rows except row 1200: 300 entries 8 columns apart (columns
    0, 8, .., 2392; its diagonal is 8 * 150).  300 entries fit the stage but 300 lines do not
    fit a tile: the row is a block of its own on the untiled path.
      rows 0..1199: 4 * 256 + 176 -> 5 blocks;  row 1200: 1 block (the block holds 300 lines,
      so row 1201 does not join);  rows 1201..2499 (1299 rows): 5 * 256 + 19 -> 6 blocks.
    12 blocks."""
    n = 2500
    rows = [np.array([i]) for i in range(n)]
    rows[1200] = 8 * np.arange(300)
    return _assemble(n, rows, np.random.default_rng(125)), 12


def _pool_matrix(n, width, pools, seed, rows_per_block):
    """Rows of `width` consecutive columns; block q (rows_per_block rows each) takes its
    off-diagonal values cyclically from pools[q], its diagonals cyclically from the powers of
    two in pools[q]."""
    rows, vals = [], []
    cnt = [0] * len(pools)
    dcnt = [0] * len(pools)
    for i in range(n):
        q = min(i // rows_per_block, len(pools) - 1)
        pool = pools[q]
        pw = [v for v in pool if v > 0 and float(v).is_integer() and (int(v) & (int(v) - 1)) == 0]
        c = _window(i, n, width, width // 2)
        v = np.empty(width)
        for k, cc in enumerate(c):
            if cc == i:
                v[k] = pw[dcnt[q] % len(pw)]
                dcnt[q] += 1
            else:
                v[k] = pool[cnt[q] % len(pool)]
                cnt[q] += 1
        rows.append(c)
        vals.append(v)
    return _assemble(n, rows, vals=vals)


def _pool(k, extra=()):
    """k distinct values: the 12 powers of two, then 3, -3, 5, -5, ... (not powers of two)."""
    out = list(extra) + [float(v) for v in POW2]
    m = 3
    while len(out) < k:
        if m & (m - 1):
            out += [float(m), float(-m)]
        m += 1
    return out[:k]


@_case("vi_table", n_vi_blocks=2)
def vi_255_256_257():
    """768 rows of 8 entries: 3 blocks of 256 rows / 2048 entries (both caps at once).  Their
    values are drawn from pools of exactly 255, 256 and 257 distinct values (1792 off-diagonal
    entries per block cycle through the whole pool): the first two are value-indexed, the
    third -- one value over the table -- streams fp64 values.  Jacobi takes 1 / a_ii from the
    table in block 1 and from the dinv stream in its neighbour, block 2.  3 blocks, 2 VI."""
    A = _pool_matrix(768, 8, [_pool(255), _pool(256), _pool(257)], 131, 256)
    return A, 3


@_case("vi_table", n_vi_blocks=1)
def vi_signed_zero():
    """512 rows of 8 entries, 2 blocks.  Both store +0.0 and -0.0 explicitly: equal as doubles,
    distinct as bit patterns.  Block 0 has 254 other values: 256 patterns, value-indexed with
    both zeros in its table.  Block 1 has 255 others: 256 distinct doubles but 257 patterns,
    not value-indexed.  2 blocks, 1 VI."""
    A = _pool_matrix(512, 8, [_pool(256, extra=(0.0, -0.0)), _pool(257, extra=(0.0, -0.0))], 132, 256)
    return A, 2


@_case("vi_table", n_vi_blocks=1)
def vi_next_to_stream():
    """512 rows of 8 entries, 2 blocks: block 0 draws from 16 values (value-indexed, 1 / a_ii
    from the table), block 1 has random values (1792 draws from 4096: far more than 256
    distinct; fp64 stream, 1 / a_ii from dinv).  2 blocks, 1 VI."""
    n = 512
    A = _pool_matrix(n, 8, [_pool(16), _pool(16)], 133, 256)
    R = _assemble(n, [_window(i, n, 8, 4) for i in range(n)], np.random.default_rng(133))
    k = A.indptr[256]
    A.data[k:] = R.data[k:]
    return A, 2


@_case("odd_offsets")
def odd_offsets():
    """n = 1000; row 0 has 2 entries, every other row 9 (odd): row_ptr[r] = 2 + 9 (r - 1) is odd
    for even r >= 2, so the plain-CSR kernel's 256-row groups 1, 2, 3 start at odd k0 (2297,
    4601, 6905) and load their first 16-byte pair from k0 - 1.  A full group has 2304 > 2048
    entries: its row sums are carried across the 2048-entry chunk boundary, which falls
    inside a row (e.g. group 1: boundary at 2296 + 2048 = 4344 = 2 + 9 * 482 + 4).  nnz =
    2 + 999 * 9 = 8993 is odd (the padding pair).
    Blocks: 2 + 227 * 9 = 2045 and one more row would be 2054: [0, 228); then 227 rows
    (2043 entries) per block: 772 = 3 * 227 + 91 -> 4 blocks.  5 blocks."""
    n = 1000
    rows = [_window(i, n, 2 if i == 0 else 9, 4) for i in range(n)]
    return _assemble(n, rows, np.random.default_rng(141)), 5


def _shape_rows(start, count, offsets, vals):
    return [start + i + offsets for i in range(count)], [vals] * count


def _shape_vals(rng, offsets):
    v = _values(rng, len(offsets))
    v[offsets == 0] = float(rng.choice(POW2))
    return v


def _template_matrix(segments, tail, seed):
    """segments: (rows, entries-per-row) runs, each row of a run with the offsets 0 .. len - 1
    and the run's own values (one shape per run); then `tail` rows storing a 4.0 diagonal."""
    rng = np.random.default_rng(seed)
    rows, vals, at = [], [], 0
    for count, ln in segments:
        off = np.arange(ln)
        r, v = _shape_rows(at, count, off, _shape_vals(rng, off))
        rows += r
        vals += v
        at += count
    for i in range(tail):
        rows.append(np.array([at + i]))
        vals.append(np.array([4.0]))
    n = at + tail
    assert max(int(c[-1]) for c in rows) < n
    return _assemble(n, rows, vals=vals)


_TPL = {"AMG_TPL_MIN_ROWS": "0"}


@_case("templates", env=_TPL, n_templates=3, template_rows=704)
def tpl_len_63_64_65():
    """AMG_TPL_MIN_ROWS=0.  Rows 0..319 share a shape of 63 entries (offsets 0..62), 320..639
    one of 64 (the longest a template holds), 640..949 one of 65 (not templated), 950..1013
    store a 4.0 diagonal (a one-entry shape).  3 templates cover 320 + 320 + 64 = 704 of 1014
    rows (>= half: used).
    Blocks also break where the template flag changes: 32 rows of 63 are 2016 entries (+ 63 >
    2048): 10 blocks; 32 rows of 64 are exactly 2048: 10 blocks; 31 rows of 65 are 2015
    (+ 65 > 2048): 310 rows -> 10 blocks; the 64 tail rows: 1 block.  31 blocks."""
    return _template_matrix([(320, 63), (320, 64), (310, 65)], 64, 151), 31


@_case("templates", env=_TPL, n_templates=16, template_rows=512)
def tpl_entries_1024():
    """AMG_TPL_MIN_ROWS=0.  16 shapes of 64 entries, 32 rows each: 16 * 64 = 1024 = kTplEntries
    template entries exactly, all 16 taken.  The 64 tail rows' one-entry shape (padded to 4
    entries) would make 1028: not templated.  512 of 576 rows templated.
    Blocks: each shape's 32 rows are 2048 entries: 16 blocks; the tail: 1.  17 blocks."""
    return _template_matrix([(32, 64)] * 16, 64, 152), 17


@_case("templates", env=_TPL, n_templates=16, template_rows=512)
def tpl_entries_1025():
    """tpl_entries_1024 with a 17th shape of 64 entries: over kTplEntries, so its 32 rows stay
    on the CSR blocks.  16 templates, 512 of 608 rows.  Blocks: 16 + 1 (the 17th shape, 2048
    entries) + 1 (tail).  18 blocks."""
    return _template_matrix([(32, 64)] * 17, 64, 153), 18


@_case("templates", env=_TPL, n_templates=255, template_rows=1020)
def tpl_shapes_300():
    """AMG_TPL_MIN_ROWS=0.  300 shapes of 2 entries (diagonal 4.0, offset +1 with value
    -(s + 1)), 4 consecutive rows each, and a last row with its diagonal only: n = 1201.  The
    first 255 = kTplMax shapes are templated (255 * 4 padded entries = 1020 <= 1024):
    1020 of 1201 rows.
    Blocks: rows 0..1019 (templated, 2 entries each): 3 * 256 + 252 -> 4 blocks; rows
    1020..1200 (181 rows, flag 0): 1 block.  5 blocks."""
    rows, vals = [], []
    for s in range(300):
        for k in range(4):
            i = 4 * s + k
            rows.append(np.array([i, i + 1]))
            vals.append(np.array([4.0, -(s + 1.0)]))
    rows.append(np.array([1200]))
    vals.append(np.array([4.0]))
    return _assemble(1201, rows, vals=vals), 5


def _block_diag(size, count, tail, seed):
    rng = np.random.default_rng(seed)
    rows, n = [], size * count + tail
    for q in range(count):
        rows += [np.arange(q * size, (q + 1) * size)] * size
    rows += [np.arange(size * count, n)] * tail
    return _assemble(n, rows, rng)


_SPLIT = {"AMG_GS_SPLIT_NPR": "0"}


def _gs_chain(w, count, tail, nb, seed, derivation):
    def build():
        return _block_diag(w + 1, count, tail, seed), nb
    build.__name__ = f"gs_chain_{w}"
    build.__doc__ = (f"Dense diagonal blocks of {w + 1} rows, laid end to end ({count} of them"
                     + (f", then one of {tail}" if tail else "") + f"): n = {(w + 1) * count + tail},"
                     f" not a multiple of 64.  Block 0 lies inside the first 64-row chunk, so its last"
                     f" row has {w} couplings to new values in a forward sweep and its first row {w} in"
                     f" a backward one; no row has more: gs_chain_maxw = {w} | {w} << 16 at B = 64"
                     f" (AMG_GS_SPLIT_NPR=0 forces the split sweep).  " + derivation)
    return _case("gs_chain", env=_SPLIT, gs_width=w)(build)


_gs_chain(8, 70, 0, 3, 161, "Rows of 9 entries: 227 per block (2043; + 9 > 2048): 630 = 227 + 227 + 176.  3 blocks.")
_gs_chain(9, 63, 0, 4, 162, "Rows of 10: 204 per block (2040): 630 = 3 * 204 + 18.  4 blocks.")
_gs_chain(16, 37, 0, 6, 163, "Rows of 17: 120 per block (2040): 629 = 5 * 120 + 29.  6 blocks.")
_gs_chain(17, 35, 0, 6, 164, "Rows of 18: 113 per block (2034): 630 = 5 * 113 + 65.  6 blocks.")
_gs_chain(32, 19, 0, 11, 165, "Rows of 33: 62 per block (2046): 627 = 10 * 62 + 7.  11 blocks.")
_gs_chain(33, 18, 0, 11, 166, "Rows of 34: 60 per block (2040): 612 = 10 * 60 + 12.  11 blocks.")
_gs_chain(63, 9, 40, 19, 167, "Rows of 64: 32 per block (exactly 2048): 576 rows -> 18 blocks; the 40-row "
          "tail block (1600 entries) -> 1.  19 blocks.")

_ELL = {"AMG_GS_SPLIT": "0", "AMG_GS_TEMPLATES": "0"}


def _ell_matrix(k, seed):
    n = 200
    return _pool_matrix(n, 130, [_pool(k)], seed, n)


@_case("gs_ell", env=_ELL, ell_wide=True, n_values=256, n_vi_blocks=14)
def gs_ell_wide_256():
    """AMG_GS_SPLIT=0, AMG_GS_TEMPLATES=0: the one-kernel sliced-ELL sweep.  200 rows of 130
    consecutive columns: every slab is 132 cells wide (>= kGsWide = 128: the wide variant).  The
    values cycle through a pool of exactly 256: the GS value dictionary is full.
    Blocks: 15 rows of 130 are 1950 entries (+ 130 > 2048): 200 = 13 * 15 + 5 -> 14 blocks,
    each with <= 256 values: 14 VI."""
    return _ell_matrix(256, 171), 14


@_case("gs_ell", env=_ELL, ell_wide=True, n_values=257, n_vi_blocks=0)
def gs_ell_wide_257():
    """gs_ell_wide_256 with a pool of 257 values: one over the GS dictionary (fp64 ELL values).
    Every block's 129 * rows off-diagonal entries (>= 645) cycle through all 257: 14 blocks,
    0 VI."""
    return _ell_matrix(257, 172), 14


@functools.lru_cache(maxsize=None)
def zoo():
    """name -> Case.  The matrices are shared: treat them as read-only."""
    out = {}
    for name, group, fn, kw in _BUILDERS:
        A, nb = fn()
        A = A.tocsr()
        assert A.has_sorted_indices or A.nnz == 0
        out[name] = Case(name=name, group=group, A=A, n_blocks=nb, doc=fn.__doc__, **kw)
    return out


def zoo_names(group=None):
    return [name for name, g, _, _ in _BUILDERS if group is None or g == group]
