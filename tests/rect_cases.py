"""Rectangular operators that sit exactly on the limits of the paths only an interpolation or a
restriction takes in csr_block_kernel -- the gather path's 2 / 4 / 8 lane slots, four rows per
lane, 16-bit column codes in bands of 16,384, packed value indices, x tiles with several rows
per lane, the rectangular tile-or-gather and line-width rules, block_long -- and the builders'
rules for them restated in plain numpy (no GPU, no oracle).  The square zoo is
tests/edge_cases.py; its exact-integer references (bits, int_vectors, exact_spmv, ...) are reused
here: every stored value is an integer with |v| <= 2^11.

The rectangular build rules (DevMatrix::build_view, choose_cut, build_row_blocks, gather_codes,
build_value_index in raptor_amd/csrc/par_matrix.hip), restated by plan():
  rows per block   rpb = 4 if nnz <= 4 n_rows else 1; a block holds at most 256 rpb rows.
  the cut          rows are taken greedily; a block is closed before row r when its entries plus
                   row r's exceed 2048, or it holds 256 rpb rows, or (line cap) its distinct x
                   lines plus row r's new ones exceed 2048 / lw, or row r's class (it reads a halo
                   column or not) differs.  A single row over a cap is a block of its own.
  lines            line_of(c) = c // lw for a local column, ceil(ncl / lw) + (c - ncl) // lw for
                   halo column c - ncl; lw = 8 doubles (64 B) or 4 (32 B).
  tile or gather   from the cut at 64-byte lines with the 256-line cap (a row over the cap counts
                   257 lines): tiled iff 2 sum(lines) <= sum(nnz).  AMG_RECT_TILE=0 / 1 forces it.
  line width       a tiled operator is cut at 32-byte lines (512-line cap) iff
                   4 sum(lines) >= 3 * 256 * n_blocks (AMG_TILE_LINE=8 / 4 forces it); no
                   block-count comparison as for square operators.
  gather re-cut    a gather operator is cut without the line cap.
  slots            a gather block's lanes hold 2 entries each if it has <= 512, 4 if <= 1024,
                   else 8.
  value index      a block of 1 .. 2048 entries with <= 256 distinct bit patterns.
  column codes     per gather block of 1 .. 2048 entries, bands over its sorted columns: a new
                   band starts at the first column c with c - base >= 16384.  More than four bands
                   in any block leaves the whole operator on 32-bit columns; AMG_GATHER_C16=0
                   turns the codes off at launch.
Blocks are stored interior first, then boundary (rows that read the halo); on one rank every
row is interior.  Every zoo operator is below 4096 rows: one chunk, the sampled cut is the
whole operator."""
import functools
from dataclasses import dataclass, field

import numpy as np
import scipy.sparse as sp

from tests.edge_cases import CAP, ROWS, bits

BAND = 1 << 14      # kGatherBand
RPB = 4             # kGatherRPB
N_ROWS_MAX, N_COLS_MAX, NNZ_MAX = 5000, 100_000, 300_000


# ---- the builders' rules, restated ----------------------------------------------------------
def line_of(c, ncl, lw):
    c = np.asarray(c, np.int64)
    return np.where(c < ncl, c // lw, -(-ncl // lw) + (c - ncl) // lw)


def gather_slots(nz):
    return 2 if nz <= 2 * ROWS else 4 if nz <= 4 * ROWS else 8


def cut(A, row_cap, lw=8, line_cap=True, ncl=None, cls=None):
    """build_row_blocks on one chunk: ([r0, r1), distinct lines) per block, in row order.
    A's columns are in local numbering (local, then halo from ncl on); cls: per-row class."""
    A = A.tocsr()
    n, rp, col = A.shape[0], A.indptr, A.indices
    ncl = A.shape[1] if ncl is None else ncl
    cap_lines = CAP // lw
    out, r0, acc, lines = [], 0, 0, set()
    for r in range(n):
        mine = set(line_of(col[rp[r]:rp[r + 1]], ncl, lw).tolist())
        ln = int(rp[r + 1] - rp[r])
        if r > r0 and ((cls is not None and cls[r] != cls[r0]) or acc + ln > CAP or r - r0 >= row_cap or
                       (line_cap and len(lines | mine) > cap_lines)):
            out.append(((r0, r), len(lines)))
            r0, acc, lines = r, 0, set()
        lines |= mine
        acc += ln
    if n > r0:
        out.append(((r0, n), len(lines)))
    return out


def block_nnz(A, blk):
    return int(A.indptr[blk[1]] - A.indptr[blk[0]])


def block_bands(A, blk):
    """Bands of gather_codes for one block: the list of band bases (greedy over sorted columns)."""
    c = np.sort(A.indices[A.indptr[blk[0]]:A.indptr[blk[1]]].astype(np.int64))
    bases = []
    for v in c.tolist():
        if not bases or v - bases[-1] >= BAND:
            bases.append(v)
    return bases


def n_values(A, blk):
    return len(np.unique(bits(A.data[A.indptr[blk[0]]:A.indptr[blk[1]]])))


def plan(A, env=None, ncl=None, cls=None):
    """What build_view makes of a rectangular A under the AMG_* knobs in env: rpb, tiled, lw,
    blocks ([r0, r1) in stored order), lines per block, n_vi, per-block band counts, c16."""
    env = env or {}
    A = A.tocsr()
    n = A.shape[0]
    rpb = RPB if A.nnz <= RPB * n else 1
    row_cap = ROWS * rpb
    s8 = cut(A, row_cap, 8, True, ncl, cls)
    lines8 = [min(ln, CAP // 8 + 1) for _, ln in s8]   # an untiled row counts cap + 1 lines
    nnz8 = sum(block_nnz(A, b) for b, _ in s8)
    mode = int(env.get("AMG_RECT_TILE", -1))
    tiled = mode != 0 and (mode == 1 or 2 * sum(lines8) <= nnz8)
    lw = 8
    if tiled and s8:
        force = int(env.get("AMG_TILE_LINE", 0))
        if force == 4 or (force != 8 and 4 * sum(lines8) >= 3 * (CAP // 8) * len(s8)):
            lw = 4
    final = cut(A, row_cap, lw, tiled, ncl, cls)
    if cls is not None:   # interior blocks first, then boundary
        final = [f for f in final if not cls[f[0][0]]] + [f for f in final if cls[f[0][0]]]
    blocks = [b for b, _ in final]
    nz = [block_nnz(A, b) for b in blocks]
    coded = [b for b, z in zip(blocks, nz) if 0 < z <= CAP]
    bands = [len(block_bands(A, b)) if 0 < z <= CAP else 0 for b, z in zip(blocks, nz)]
    c16_built = (not tiled) and len(blocks) > 0 and all(len(block_bands(A, b)) <= 4 for b in coded)
    return dict(rpb=rpb, tiled=tiled, lw=lw, blocks=blocks, lines=[ln for _, ln in final], nnz=nz,
                n_vi=sum(1 for b in coded if n_values(A, b) <= 256), bands=bands,
                slots=[gather_slots(z) if 0 < z <= CAP else 0 for z in nz],
                c16=c16_built and env.get("AMG_GATHER_C16", "1") != "0",
                tile_line_bytes=8 * lw if tiled else 0)


# ---- the zoo ---------------------------------------------------------------------------------
@dataclass
class Case:
    name: str
    group: str
    A: sp.csr_matrix
    n_blocks: int                 # hand-derived (the builder's docstring)
    n_vi_blocks: int
    tiled: bool
    c16: bool
    tile_line_bytes: int          # 0: gather
    rpb: int
    block_nnz: list = None        # entries per block, where the docstring derives them
    bands: list = None            # bands per block, where the docstring derives them
    env: dict = field(default_factory=dict)  # AMG_* knobs set before from_csr_rect
    auto: bool = False            # the case is about the automatic choice: its own env only
    doc: str = ""
    poison: tuple = ()            # columns worth poisoning beyond 0 and n_cols - 1
    long_rows: tuple = ()


_BUILDERS = []


def _case(group, **kw):
    def deco(fn):
        _BUILDERS.append((fn.__name__, group, fn, kw))
        return fn
    return deco


def _pool(k, extra=()):
    """k distinct integer values of |v| <= 2^11: extra, then 1, -1, 2, -2, ..."""
    out = list(extra)
    m = 1
    while len(out) < k:
        out += [float(m), float(-m)]
        m += 1
    return np.array(out[:k])


def _cycle(nnz, k=300, start=0, extra=()):
    """nnz values cycling through a pool of k: any run of >= k entries holds all k."""
    return _pool(k, extra)[(start + np.arange(nnz)) % k]


def _csr(nr, nc, rows, vals=None):
    """CSR of shape (nr, nc) (nc None: up to the last column used) from per-row ascending column arrays; values: one flat array in
    entry order, or a pool of 300 cycled (no run of 300 entries is value-indexed)."""
    assert len(rows) == nr
    if nc is None:   # the last column is the last one used
        nc = 1 + max(int(c[-1]) for c in rows if len(c))
    rp = np.zeros(nr + 1, np.int64)
    rp[1:] = np.cumsum([len(c) for c in rows])
    col = np.concatenate([np.asarray(c, np.int64) for c in rows]) if rp[-1] else np.zeros(0, np.int64)
    val = _cycle(int(rp[-1])) if vals is None else np.asarray(vals, np.float64)
    assert val.size == rp[-1] and np.abs(val).max(initial=0) <= 1 << 11
    assert all(np.all(np.diff(c) > 0) for c in rows if len(c) > 1), "columns must ascend"
    assert col.size == 0 or (col.min() >= 0 and col.max() < nc)
    return sp.csr_matrix((val, col.astype(np.int32), rp.astype(np.int32)), shape=(nr, nc))


def _scatter(lens, stride=8, first=0):
    """Rows of the given lengths whose k-th entry overall sits in column first + stride k + k % 8
    (stride >= 8 a multiple of 8): every entry on a 64-byte line of its own, ascending."""
    rows, k = [], 0
    for ln in lens:
        j = np.arange(k, k + ln)
        rows.append(first + stride * j + j % 8)
        k += ln
    return rows


@_case("slots", block_nnz=[512, 513, 1024, 1025, 2048], bands=[1, 1, 1, 1, 2])
def slots_512_to_2048():
    """1280 rows in five runs of 256: row lengths 2; 2 with one row of 3; 4; 4 with one row of 5;
    8.  nnz = 512 + 513 + 1024 + 1025 + 2048 = 5122 > 4 * 1280: rpb = 1, 256 rows per block.  Every
    entry has a 64-byte line of its own (column 8 k + k % 8 for entry k), so the sampled cut
    counts 5122 lines: 2 * 5122 > 5122, gather.  Without the line cap only the row cap cuts
    (the last run also fills the entry cap): 5 blocks of 512, 513, 1024, 1025 and 2048 entries --
    2, 4, 4, 8 and 8 lane slots, each on the edge of its slot count.  The last entry of the last
    block is the operator's last and is moved to column n_cols - 1 = 69,999.  Columns: a block of z
    entries spans 8 z <= 16,384 columns: one band each; the last block's entries but the moved one
    end at offset 8 * 2046 + 0 = 16,368 from its base 24,592, and 69,999 starts a second band.
    No block is value-indexed (any 300 consecutive entries hold 300 values)."""
    lens = [2] * 256 + [2] * 255 + [3] + [4] * 256 + [4] * 255 + [5] + [8] * 256
    rows = _scatter(lens)
    rows[-1] = np.append(rows[-1][:-1], 69_999)
    return _csr(1280, 70_000, rows), dict(n_blocks=5, n_vi_blocks=0, tiled=False, c16=True,
                                           tile_line_bytes=0, rpb=1)


def _rpb4_lens():
    rng = np.random.default_rng(201)

    def mix(n4, n1, n0, first=None, last=None):
        v = np.array([4] * n4 + [1] * n1 + [0] * n0)
        rng.shuffle(v)
        v = v.tolist()
        for pos, want in ((0, first), (-1, last)):   # pin an end: swap with a row of that length
            if want is not None and v[pos] != want:
                j = v.index(want, 1, len(v) - 1)
                v[pos], v[j] = v[j], v[pos]
        return v
    a = mix(400, 446, 177)                # 1023 rows, 2046 entries
    b = mix(300, 500, 224, first=4)       # 1024 rows, 1700 entries, first row 4: 2046 + 4 > 2048
    c = mix(300, 500, 224)                # 1024 rows, 1700 entries
    d = [4] * 512                         # 2048 entries
    e = mix(300, 500, 224, first=1)       # 1024 rows, first row 1: 2048 + 1 > 2048
    return a + b + c + d + e + [1]


@_case("rpb4", block_nnz=[2046, 1700, 1700, 2048, 1700, 1])
def rpb4_rows():
    """4608 rows of 0, 1 and 4 entries mixed, nnz = 9195 <= 4 * 4608: rpb = 4, up to 1024 rows per
    block; every entry on a line of its own: gather.
      rows 0..1022 (400 of 4, 446 of 1, 177 empty): 2046 entries; row 1023 has 4 -> 2050 > 2048:
        a block of 1023 rows (lane 255 has no fourth row).
      rows 1023..2046 (1024 rows, 1700 entries): closed by the row cap at exactly 1024 rows.
      rows 2047..3070 (1024 rows, 1700 entries) and 512 rows of 4 after them: the 1025th row
        spills into a new block, which the entry cap closes at 512 rows of 4 = 2048 entries
        (the lanes' third and fourth rows are absent).
      rows 3583..4606 (1024 rows, 1700 entries, the first has 1: 2048 + 1 > 2048): row cap.
      row 4607 (1 entry): the operator's last block is a single row, value-indexed.
    6 blocks, 1 VI.  Lanes' 2nd to 4th rows are present, absent or empty throughout."""
    lens = _rpb4_lens()
    return _csr(4608, None, _scatter(lens)), dict(n_blocks=6, n_vi_blocks=1, tiled=False, c16=True,
                                                     tile_line_bytes=0, rpb=4)


@_case("empty", block_nnz=[1024, 0, 100])
def empty_rpb4():
    """2148 rows: 1024 of one entry, 1024 empty, 100 of one entry; nnz = 1124 <= 4 n: rpb = 4.
    Every entry on its own line: gather.  The row cap cuts [0, 1024), [1024, 2048) -- an
    nnz == 0 block between two non-empty ones, block_long's empty path over 1024 rows -- and
    [2048, 2148), 100 entries of 100 values: value-indexed, its index offset skips both blocks
    before it.  3 blocks, 1 VI."""
    lens = [1] * 1024 + [0] * 1024 + [1] * 100
    return _csr(2148, None, _scatter(lens)), dict(n_blocks=3, n_vi_blocks=1, tiled=False, c16=True,
                                                   tile_line_bytes=0, rpb=4)


@_case("empty", block_nnz=[2048, 0, 2048])
def empty_rpb1():
    """768 rows: 256 of 8 entries, 256 empty, 256 of 8; nnz = 4096 > 4 * 768: rpb = 1.  Gather (a
    line per entry).  [0, 256) is full in rows and entries, [256, 512) is an nnz == 0 block,
    [512, 768).  3 blocks, 0 VI."""
    lens = [8] * 256 + [0] * 256 + [8] * 256
    return _csr(768, None, _scatter(lens)), dict(n_blocks=3, n_vi_blocks=0, tiled=False, c16=True,
                                                    tile_line_bytes=0, rpb=1)


@_case("empty", block_nnz=[0, 0])
def empty_nnz0():
    """1500 x 37 with no entry at all.  nnz = 0 <= 4 n: rpb = 4; the sampled cut has 0 lines and 0
    entries, 2 * 0 <= 0: tiled, and 4 * 0 < 3 * 256 * 2: 64-byte lines.  The row cap cuts
    [0, 1024), [1024, 1500): 2 empty blocks, nothing to index or code."""
    return _csr(1500, 37, [np.zeros(0, np.int64)] * 1500), dict(n_blocks=2, n_vi_blocks=0, tiled=True,
                                                                  c16=False, tile_line_bytes=64, rpb=4)


def _long_matrix():
    lens = [8] * 256 + [0] + [8] * 256 + [0] + [8] * 256
    rows = _scatter(lens)
    rows[256] = 30_000 + np.arange(2049)
    rows[513] = 3 + 17 * np.arange(4097)
    return _csr(770, 70_000, rows)


@_case("long", block_nnz=[2048, 2049, 2048, 4097, 2048], poison=(30_000, 3 + 17 * 4096),
       long_rows=(256, 513))
def long_gather():
    """770 rows: three runs of 256 rows of 8 scattered entries (a line each, columns below
    49,152), row 256 with 2049 consecutive columns from 30,000 and row 513 with 4097 columns 17
    apart (3 .. 69,635: five bands' worth).  nnz = 12,290 > 4 n: rpb = 1.  Sampled cut: 6144
    lines of the short rows + 257 for each long row (over the line cap); 2 * 6658 > 12,290:
    gather.  Each long row exceeds the entry cap and is a block of its own on block_long, which
    reads 32-bit columns; the other three blocks (2048 entries within 16,384 + 7 columns: 2
    bands at most) read 16-bit codes -- the rule skips blocks over 2048 entries, so the codes
    stay on.  5 blocks, 0 VI."""
    return _long_matrix(), dict(n_blocks=5, n_vi_blocks=0, tiled=False, c16=True, tile_line_bytes=0, rpb=1)


@_case("long", env={"AMG_RECT_TILE": "1"}, poison=(30_000, 3 + 17 * 4096), long_rows=(256, 513))
def long_tiled():
    """long_gather's operator forced onto x tiles (AMG_RECT_TILE=1).  Sampled cut at 64-byte
    lines: a short row has 8 lines, 32 rows fill the 256-line cap: 24 blocks of 256 lines + the
    two long rows at 257: 4 * 6658 >= 3 * 256 * 26: 32-byte lines.  There a short row still has
    8 lines of its own, 64 rows fill the 512-line cap: 4 + 1 + 4 + 1 + 4 = 14 blocks; the long
    rows are untiled blocks (block_long) between tile blocks.  0 VI (512 entries per block cycle
    300 values)."""
    return _long_matrix(), dict(n_blocks=14, n_vi_blocks=0, tiled=True, c16=False, tile_line_bytes=32, rpb=1)


@_case("long", auto=True, block_nnz=[2048, 257, 2048], poison=(8 * 256,), long_rows=(256,))
def long_untiled_row():
    """513 rows x 2049: rows 0..255 and 257..512 hold 8 consecutive columns from 8 * (i // 4) (four
    rows share a line: 64 lines per 256 rows), row 256 holds 257 entries 8 columns apart: 257
    lines of 64 B, one more than a tile.  nnz = 4353 > 4 n: rpb = 1.  Sampled cut: [0, 256) by the
    row cap (64 lines), row 256 alone (257), [257, 513) (64 lines): 2 * 385 <= 4353: tiled;
    4 * 385 < 3 * 256 * 3: 64-byte lines.  The middle block has <= 2048 entries but no tile: an
    untiled block (block_long) inside a tiled operator.  3 blocks; the middle one's 257 entries
    are 257 consecutive values of the cycle of 300, one over the table: 0 VI."""
    rows = []
    for i in range(513):
        j = i if i < 256 else i - 1
        rows.append(8 * np.arange(257) if i == 256 else 8 * (j // 4) + np.arange(8))
    return _csr(513, None, rows), dict(n_blocks=3, n_vi_blocks=0, tiled=True, c16=False, tile_line_bytes=64, rpb=1)


def _band_block(bases, counts, last_offsets):
    """Sorted columns of one 256-row block: per band `count` entries 8 apart from its base, the
    last moved to base + last_offset (None: left)."""
    c = []
    for b, n, lo in zip(bases, counts, last_offsets):
        v = b + 8 * np.arange(n)
        if lo is not None:
            v[-1] = b + lo
        c.append(v)
    c = np.concatenate(c)
    assert c.size == 2048 and np.all(np.diff(c) > 0)
    return [c[8 * i:8 * i + 8] for i in range(256)]


def _bands_case(blocks):
    rows = [r for b in blocks for r in b]
    return _csr(len(rows), 70_000, rows)


_GATHER = dict(tiled=False, tile_line_bytes=0, rpb=1, n_vi_blocks=0)


@_case("bands", bands=[1, 1], poison=(1000, 1000 + 16_383, 40_000))
def bands_offset_16383():
    """Two blocks of 256 rows of 8 (2048 entries, a line each: gather, rpb = 1).  Block 0: columns
    1000 + 8 j, the last at 1000 + 16383: the largest offset a band holds -- one band, whose base
    is not 0, so the three unused bases repeat it.  Block 1: one band from 40,000."""
    A = _bands_case([_band_block([1000], [2048], [16_383]), _band_block([40_000], [2048], [None])])
    return A, dict(n_blocks=2, c16=True, **_GATHER)


@_case("bands", bands=[2, 1], poison=(1000, 1000 + 16_384, 40_000))
def bands_offset_16384():
    """bands_offset_16383 with block 0's last column one further, at offset 16384: a second band
    that starts there and holds that entry alone."""
    A = _bands_case([_band_block([1000], [2048], [16_384]), _band_block([40_000], [2048], [None])])
    return A, dict(n_blocks=2, c16=True, **_GATHER)


_B4 = [0, 17_000, 34_000, 51_000]


@_case("bands", bands=[4, 2], poison=tuple(_B4) + tuple(b + 16_383 for b in _B4) + (20_000, 53_616))
def bands_four():
    """Block 0: four bands from 0, 17,000, 34,000 and 51,000, 512 entries each, each band's last
    entry at offset 16383 (column 0 is used; the last is 67,383).  Block 1: bands from 20,000 and
    53,616, the second's last entry at offset 16383 = column n_cols - 1 = 69,999.  At most four
    bands everywhere: codes on (kernel_variant & 256)."""
    A = _bands_case([_band_block(_B4, [512] * 4, [16_383] * 4),
                     _band_block([20_000, 53_616], [1024, 1024], [None, 16_383])])
    return A, dict(n_blocks=2, c16=True, **_GATHER)


_B5 = [0, 16_400, 32_800, 49_200, 65_600]


@_case("bands", bands=[5, 2], poison=tuple(_B5) + tuple(b + 16_383 for b in _B5[:4]) + (20_000, 53_616))
def bands_five():
    """bands_four with a fifth band in block 0 (bases 0, 16,400, 32,800, 49,200, 65,600; 410
    entries in each of the first four, their last at offset 16383, and 408 in the fifth): one
    block over four bands leaves the whole operator, block 1 included, on 32-bit columns
    (kernel_variant & 256 clear)."""
    A = _bands_case([_band_block(_B5, [410] * 4 + [408], [16_383] * 4 + [None]),
                     _band_block([20_000, 53_616], [1024, 1024], [None, 16_383])])
    return A, dict(n_blocks=2, c16=False, **_GATHER)


@_case("vi", block_nnz=[512, 512, 512, 1024, 1024, 1024, 2048, 2048, 2048, 1])
def vi_slots():
    """2305 rows: nine runs of 256 rows with 2, 2, 2, 4, 4, 4, 8, 8, 8 entries per row, then one row
    of one entry; nnz = 10,753 > 4 n: rpb = 1; a line per entry: gather; the row cap cuts 9 blocks
    of 512 / 1024 / 2048 entries (2, 4, 8 slots, three of each) and the last row alone.  Per slot
    count the three blocks cycle pools of 255, 257 and 256 values: indexed, streamed, indexed --
    the streamed block sits between two indexed ones, so the packed index offsets skip it.  The
    256-value pools hold +0.0 and -0.0 as two table entries.  The last block is an indexed block
    of one entry.  10 blocks, 7 VI."""
    lens, vals = [], []
    for ln in (2, 4, 8):
        for k in (255, 257, 256):
            lens += [ln] * 256
            vals.append(_cycle(256 * ln, k, extra=(0.0, -0.0) if k == 256 else ()))
    lens.append(1)
    vals.append(np.array([7.0]))
    A = _csr(2305, None, _scatter(lens), np.concatenate(vals))
    return A, dict(n_blocks=10, n_vi_blocks=7, tiled=False, c16=True, tile_line_bytes=0, rpb=1)


def _tile_rule_rows():
    return [np.array([8 * i, 8 * i + 1]) for i in range(1024)]


@_case("tile_rule", auto=True, block_nnz=[1024, 1024])
def tile_rule_tiled():
    """1024 rows of 2 entries in columns {8 i, 8 i + 1}; nnz = 2048 <= 4 n: rpb = 4.  Sampled cut: a
    line per row, the 256-line cap cuts 4 blocks of 256 rows: 2 * 1024 == 2048: tiled, on the
    edge.  4 * 1024 >= 3 * 256 * 4: 32-byte lines, where a row still has one line: 512 rows per
    block.  2 blocks."""
    return _csr(1024, None, _tile_rule_rows()), dict(n_blocks=2, n_vi_blocks=0, tiled=True, c16=False,
                                                      tile_line_bytes=32, rpb=4)


@_case("tile_rule", auto=True, block_nnz=[2048], bands=[1])
def tile_rule_gather():
    """tile_rule_tiled with the last entry moved to column 8199 = n_cols - 1, a fresh line (1024):
    row 1023 now has two lines and is cut off the fourth sampled block: 256 * 3 + 255 + 2 = 1025
    lines, 2 * 1025 = 2048 + 2 > 2048: gather.  Without the line cap the row cap and the entry cap
    both close the one block of 1024 rows and 2048 entries (8 slots, 4 rows per lane, one band)."""
    rows = _tile_rule_rows()
    rows[-1] = np.array([8184, 8199])
    return _csr(1024, 8200, rows), dict(n_blocks=1, n_vi_blocks=0, tiled=False, c16=True,
                                         tile_line_bytes=0, rpb=4)


@_case("tile_rpb4", auto=True, block_nnz=[512, 1024, 2048, 10])
def tile_rpb4_caps():
    """1802 rows x 4114, nnz = 3594 <= 4 n: rpb = 4.
      rows 0..255: columns {8 i, 8 i + 1}, a line each: 256 lines; row 256 brings a new line:
        closed by the line cap at 256 rows, before the row cap.
      rows 256..1279: one entry each in consecutive columns 2048..3071 (128 lines, 1024 entries):
        closed by the row cap at exactly 1024 rows.
      rows 1280..1791: 4 consecutive columns from 3072 + 2 j (columns 3072..4097: 129 lines): 512
        rows of 4 = 2048 entries; the next row does not fit: closed by the entry cap.
      rows 1792..1801: one entry each in columns 4104..4113 (2 lines), 10 values: value-indexed.
    Lines 256 + 128 + 129 + 2 = 515: 2 * 515 <= 3594: tiled; 4 * 515 < 3 * 256 * 4: 64-byte lines.
    4 blocks, 1 VI."""
    rows = [np.array([8 * i, 8 * i + 1]) for i in range(256)]
    rows += [np.array([2048 + j]) for j in range(1024)]
    rows += [3072 + 2 * j + np.arange(4) for j in range(512)]
    rows += [np.array([4104 + j]) for j in range(10)]
    return _csr(1802, 4114, rows), dict(n_blocks=4, n_vi_blocks=1, tiled=True, c16=False,
                                         tile_line_bytes=64, rpb=4)


def _tile_width(lines2):
    rows = [np.array([4 * i, 4 * i + 1]) for i in range(512)]
    rows += [np.array([2048 + min(j, 8 * lines2 - 1)]) for j in range(1024)]
    return _csr(1536, 3072, rows)


@_case("tile_width", auto=True, block_nnz=[1024, 1024])
def tile_width_32():
    """1536 rows x 3072, nnz = 2048 <= 4 n: rpb = 4.  Rows 0..511: columns {4 i, 4 i + 1}; rows
    512..1535: one entry each in columns 2048..3071.  Sampled cut at 64-byte lines: two rows
    share a line, 512 rows fill the 256-line cap and row 512 brings a 257th: [0, 512) with 256
    lines, [512, 1536) with 128: 2 * 384 <= 2048: tiled; 4 * 384 == 3 * 256 * 2: 32-byte lines, on
    the edge.  There rows 0..511 have a line each: exactly 512 lines, and row 512 would be the
    513th: [0, 512) is a full tile closed by the line cap; [512, 1536) has 256 lines and exactly
    1024 rows.  2 blocks."""
    return _tile_width(128), dict(n_blocks=2, n_vi_blocks=0, tiled=True, c16=False, tile_line_bytes=32, rpb=4)


@_case("tile_width", auto=True, block_nnz=[1024, 1024])
def tile_width_64():
    """tile_width_32 with one line fewer: the last 9 rows all store column 3063 (the last of line
    382; the operator's last line is unused).  383 lines: 4 * 383 < 3 * 256 * 2: 64-byte lines,
    the sampled cut's own 2 blocks."""
    return _tile_width(127), dict(n_blocks=2, n_vi_blocks=0, tiled=True, c16=False, tile_line_bytes=64, rpb=4)


def _narrow(nc):
    def build():
        rows = [np.unique([i % nc, nc - 1]) for i in range(1030)]
        return _csr(1030, nc, rows), dict(n_blocks=2, n_vi_blocks=1, tiled=True, c16=False,
                                          tile_line_bytes=64, rpb=4)
    build.__name__ = f"narrow_{nc}"
    build.__doc__ = (f"1030 rows x {nc}: row i stores columns i % {nc} and {nc - 1} (one entry where they "
                     f"coincide), so the last column of an x of {nc} entries is read by every row.  nnz <= "
                     f"2 n: rpb = 4; at most {-(-nc // 8)} lines per block: tiled, 64-byte lines.  The row cap "
                     f"cuts [0, 1024) (<= 2048 entries) and [1024, 1030) (<= 12 entries: value-indexed).  "
                     f"2 blocks, 1 VI." + ("  n_cols == 1: the x tile's 8-byte loads (wide_x == 0)." if nc == 1 else ""))
    return _case("narrow", auto=False)(build)


for _nc in (1, 2, 3, 7, 9, 257):
    _narrow(_nc)


@functools.lru_cache(maxsize=None)
def zoo():
    """name -> Case.  The matrices are shared: treat them as read-only."""
    out = {}
    for name, group, fn, kw in _BUILDERS:
        A, claims = fn()
        A = A.tocsr()
        assert A.has_sorted_indices or A.nnz == 0
        assert A.shape[0] <= N_ROWS_MAX and A.shape[1] <= N_COLS_MAX and A.nnz <= NNZ_MAX
        out[name] = Case(name=name, group=group, A=A, doc=fn.__doc__, **claims, **kw)
    return out


def zoo_names(group=None):
    return [name for name, g, _, _ in _BUILDERS if group is None or g == group]


def run_envs(c):
    """The environments a case runs under: its own, and -- unless it is about the automatic
    choice or forces the choice itself -- the codes off and the tile choice forced both ways."""
    envs = {"own": dict(c.env)}
    if not c.auto and not c.env:
        envs["c16_off"] = {"AMG_GATHER_C16": "0"}
        envs["gather"] = {"AMG_RECT_TILE": "0"}
        envs["tile"] = {"AMG_RECT_TILE": "1"}
    return envs


def poison_columns(c):
    """Columns 0 and n_cols - 1, the case's own (band bases, base + 16383, a long row's), and one
    in the middle of the columns used."""
    nc = c.A.shape[1]
    used = np.unique(c.A.indices)
    mid = [int(used[used.size // 2])] if used.size else []
    return sorted({0, nc - 1, *mid, *(int(p) for p in c.poison if p < nc)})


# ---- one changed entry (the checks' own sensitivity) --------------------------------------------
def mutate(A, how):
    """(A', affected row): one value + 1, one entry dropped, or -- on a block whose last column
    sits at offset 16383 of its band -- that column moved to offset 16384 (into a new band)."""
    A = A.copy()
    ln = np.diff(A.indptr)
    rows = np.flatnonzero(ln >= 2)
    r = int(rows[len(rows) // 2])
    k = A.indptr[r] + 1
    if how == "value":
        A.data[k] += 1.0
    elif how == "drop":
        assert A.data[k] != 0.0
        keep = np.ones(A.nnz, bool)
        keep[k] = False
        rp = A.indptr.copy()
        rp[r + 1:] -= 1
        A = sp.csr_matrix((A.data[keep], A.indices[keep], rp), shape=A.shape)
    else:
        base = int(A.indices[0])
        k = int(np.flatnonzero(A.indices[:A.indptr[256]] == base + BAND - 1)[0])
        r = int(np.searchsorted(A.indptr, k, side="right") - 1)
        assert k + 1 == A.indptr[r + 1] or A.indices[k + 1] > base + BAND
        A.indices[k] = base + BAND
    return A, r


# ---- several ranks: independent row and column partitions ---------------------------------------
@dataclass
class RankCase:
    name: str
    A: sp.csr_matrix              # the global operator
    row_starts: list
    col_starts: list
    doc: str = ""


def local_view(c, rank):
    """Rank `rank`'s rows of a RankCase: (rows with global columns, the same rows in the
    builder's local numbering [local | halo, halo sorted by global id], n_local_cols, halo global
    ids, per-row class: 1 = the row reads a halo column)."""
    r0, r1 = c.row_starts[rank], c.row_starts[rank + 1]
    c0, c1 = c.col_starts[rank], c.col_starts[rank + 1]
    G = c.A[r0:r1].tocsr()
    G.sort_indices()
    g = G.indices.astype(np.int64)
    mine = (g >= c0) & (g < c1)
    halo = np.unique(g[~mine])
    loc = np.where(mine, g - c0, (c1 - c0) + np.searchsorted(halo, g))
    L = sp.csr_matrix((G.data, loc.astype(np.int32), G.indptr), shape=(r1 - r0, (c1 - c0) + halo.size))
    cls = np.zeros(r1 - r0, np.uint8)
    rows = np.repeat(np.arange(r1 - r0), np.diff(G.indptr))
    cls[rows[~mine]] = 1
    return G, L, c1 - c0, halo, cls


def _global(nr, nc, rows):
    rows = [np.unique(np.asarray(r, np.int64)) for r in rows]
    return _csr(nr, nc, rows)


def rank_band_across_halo():
    """Two ranks, 512 rows each; columns [0, 20001) and [20001, 40002): both own an odd number.
    Each rank's rows 0..255 are interior -- three scattered local columns 3000 + 24 i + {0, 8, 16}
    and local column 19,901 + i % 100 -- and its rows 256..511 store the same and its halo: rank 0
    reads global column 30,000 (n_halo == 1), rank 1 global columns 19,999 and 20,000
    (n_halo == 2).  nnz > 4 n: rpb = 1; >= 781 lines for <= 1536 entries per block: gather.  In
    local numbering the halo follows column 20,000 directly, so each boundary block has two
    bands: [3000, ..) and one that starts at local column 19,901 (>= 16,384 past 3000), runs to the
    last local columns and on into the halo at 20,001 (and 20,002)."""
    ncl = 20_001
    rows = []
    for rank in (0, 1):
        c0 = rank * ncl
        halo = [30_000] if rank == 0 else [19_999, 20_000]
        for i in range(512):
            j = i % 256
            r = [c0 + 3000 + 24 * j + d for d in (0, 8, 16)] + [c0 + 19_901 + j % 100]
            rows.append(r + (halo if i >= 256 else []))
    return RankCase("band_across_halo", _global(1024, 2 * ncl, rows), [0, 512, 1024], [0, ncl, 2 * ncl],
                    rank_band_across_halo.__doc__)


def rank_tiled_halo_tail():
    """Two ranks, 385 rows each; columns [0, 2049) and [2049, 4104): 2049 % 8 == 1 and 2055 % 8 == 7,
    so the last local line is partial (one column, seven columns) and the first halo line starts
    a new one.  Per rank: rows 0..255 interior, 8 consecutive local columns from 8 (i // 4) (64
    lines); rows 256..383 boundary, 4 local columns from 8 (64 + j) and the 8 halo columns from halo
    index 8 j: one local and one halo line each, 128 rows fill exactly the 256 lines of a tile;
    row 384 stores the last 8 local columns (the partial last line among them) and halo index
    1024: new lines, cut off by the line cap into a block of its own.  nnz > 4 n: rpb = 1;
    2 * (64 + 256 + 3) <= 3593: tiled; 4 * 323 < 3 * 256 * 3: 64-byte lines.  3 blocks per rank."""
    ncls = (2049, 2055)
    firsts = (0, 2049)
    rows = []
    for rank in (0, 1):
        c0, ncl, h0 = firsts[rank], ncls[rank], firsts[1 - rank]   # halo index k = global h0 + k
        for i in range(256):
            rows.append(c0 + 8 * (i // 4) + np.arange(8))
        for j in range(128):
            rows.append(np.concatenate([c0 + 8 * (64 + j) + np.arange(4), h0 + 8 * j + np.arange(8)]))
        rows.append(np.concatenate([c0 + ncl - 8 + np.arange(8), [h0 + 1024]]))
    return RankCase("tiled_halo_tail", _global(770, 4104, rows), [0, 385, 770], [0, 2049, 4104],
                    rank_tiled_halo_tail.__doc__)


def rank_missing_owners():
    """Three ranks: rank 0 owns rows [0, 300) and no column (every column it reads is halo: what a
    rank without coarse points is to R), rank 1 rows [300, 600) and columns [0, 500), rank 2 no
    row and columns [500, 1000) (what such a rank is to P).  Six columns per row, from both
    column owners."""
    rng = np.random.default_rng(301)
    rows = [np.concatenate([rng.choice(500, 3, replace=False), 500 + rng.choice(500, 3, replace=False)])
            for _ in range(600)]
    rows[0][-1] = 999
    rows[1][0] = 0
    return RankCase("missing_owners", _global(600, 1000, rows), [0, 300, 600, 600], [0, 0, 500, 1000],
                    rank_missing_owners.__doc__)


@functools.lru_cache(maxsize=None)
def rank_cases():
    return {c.name: c for c in (rank_band_across_halo(), rank_tiled_halo_tail(), rank_missing_owners())}
