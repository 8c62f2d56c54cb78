"""Helpers of the C-ABI vector contract tests (include/raptor_amd.h, "Vectors"): an arena that
places every operand of a call inside one device allocation with guard bands around it, the
contract's range predicate, and the partial sums amg_vector_read must leave.  numpy only at
module level (the arena imports torch when it uploads); tests/test_vector_contract_cpu.py shows
on the CPU that each helper can fail, tests/test_gpu_vector_contract.py runs the product on them.

Arena.  Operands are laid out one after the other, each body preceded and followed by G = 2048
doubles of guard (>= kCAP entries of a row block and >= four 512-row template groups: a store or
a load that is off by a whole block, tile or window still lands in a guard).  An operand's body
starts at an arena index with a chosen remainder modulo 8, so that its address is 16-byte
aligned (even start), only 8-byte aligned (odd start) or 7 mod 8.
  * input guards hold NaN: an out-of-range read that reaches a product makes a row non-finite;
  * output guards, and output bodies that have no initial data, hold canary(i): a quiet NaN
    whose payload carries the arena index i, so a store that is shifted or duplicated from
    elsewhere in the arena is noticed as well as one with fresh data.
check() returns the arena indices of guard words that changed, inputs_changed() those of input
body words, untouched(name) whether an output body still holds its canaries."""
import numpy as np

G = 2048
NAN_BITS = np.uint64(0x7FF8000000000000)
CANARY_TAG = np.uint64(0x7FFC5A0000000000)   # quiet NaN, payload tag 0xC5A in bits 50..40

# amg_vector_copy / _read: both split a full-workgroup path from a tail path at multiples of
# 2048 doubles (1024 pairs); odd sizes take copy's one-double memcpy
COPY_SIZES = [0, 1, 2, 3, 2047, 2048, 2049, 4095, 4096, 4097, 3 * 2048 + 1023]
# amg_vector_uniform: one workgroup's edge, and one size past the 4096 x 256 lanes of the
# largest grid (the grid-stride loop)
UNIFORM_SIZES = [0, 1, 255, 256, 257]
UNIFORM_STRIDE_SIZE = 4096 * 256 + 257
UNIFORM_GIDS = [0, 1, 2 ** 40 + 3]
UNIFORM_SEEDS = [0, 42, 2 ** 63 + 11]


def read_data(n, seed=5):
    """Integers in +-2^20: every partial sum is exact in any order.  For odd n the last element
    is NaN: it belongs to no pair."""
    v = np.random.default_rng(seed).integers(-(1 << 20), (1 << 20) + 1, n).astype(np.float64)
    if n & 1:
        v[-1] = np.nan
    return v


def canary(idx):
    """The canary bit pattern of arena index idx (array or int): below 2^40 words."""
    idx = np.asarray(idx, np.uint64)
    return CANARY_TAG | idx


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def overlaps(a0, na, b0, nb):
    """The contract's predicate on half-open ranges [a0, a0 + na), [b0, b0 + nb): an empty range
    overlaps nothing."""
    return na > 0 and nb > 0 and a0 < b0 + nb and b0 < a0 + na


def read_partial_count(n):
    """Slots amg_vector_read needs for n doubles: 4 per 1024 pairs, at least 4."""
    npair = n // 2
    return 4 * max(1, -(-npair // 1024))


def read_partials_expected(src):
    """The partials amg_vector_read leaves for src: workgroup b of 256 lanes covers the pairs
    [1024 b, 1024 (b + 1)), lane t the pairs 1024 b + t + 256 u; slot 4 b + w is the sum of wave
    w's lanes, that is of the pairs p with ((p - 1024 b) % 256) // 64 == w.  The order inside a
    slot is the kernel's business: use data whose sums are exact (small integers).  An odd last
    element belongs to no pair."""
    src = np.asarray(src, np.float64)
    npair = src.size // 2
    out = np.zeros(read_partial_count(src.size))
    if npair == 0:
        return out
    pair = src[:2 * npair].reshape(npair, 2).sum(axis=1)
    p = np.arange(npair)
    slot = 4 * (p // 1024) + ((p % 1024) % 256) // 64
    np.add.at(out, slot, pair)
    return out


class Arena:
    def __init__(self, guard=G):
        self.guard = guard
        self.size = 0
        self.ops = {}       # name -> (start, n, is_output)
        self._fill = []     # (start, n, bits)
        self.image = None   # the host image as uploaded (uint64)
        self.dev = None
        self.host = None    # the last download (uint64)

    # ---- layout ------------------------------------------------------------------------------
    def _place(self, name, n, start_mod, is_output):
        assert name not in self.ops and self.image is None
        s = self.size + self.guard
        s += (start_mod - s) % 8
        self.ops[name] = (s, int(n), is_output)
        self.size = s + int(n) + self.guard
        return s

    def input(self, name, data, start_mod=0):
        data = np.ascontiguousarray(data, np.float64)
        s = self._place(name, data.size, start_mod, False)
        self._fill.append((s, data.size, bits(data).copy()))
        return self

    def output(self, name, n, start_mod=0, init=None):
        """An output body of n doubles; init: its data before the call (an in-out operand)."""
        s = self._place(name, n, start_mod, True)
        if init is not None:
            init = np.ascontiguousarray(init, np.float64)
            assert init.size == n
            self._fill.append((s, n, bits(init).copy()))
        return self

    def start(self, name):
        return self.ops[name][0]

    def build_image(self):
        img = canary(np.arange(self.size))
        for s, n, out in self.ops.values():
            if not out:
                img[s - self.guard:s] = NAN_BITS
                img[s + n:s + n + self.guard] = NAN_BITS
        for s, n, b in self._fill:
            img[s:s + n] = b
        self.image = img
        self.host = img.copy()
        return img

    # ---- device ------------------------------------------------------------------------------
    def upload(self, ctx):
        import torch

        img = self.build_image()
        with torch.cuda.stream(ctx.stream):
            self.dev = torch.from_numpy(img.view(np.float64).copy()).to(ctx.torch_device)
        ctx.stream.synchronize()
        return self

    def __getitem__(self, name):
        s, n, _ = self.ops[name]
        return self.dev[s:s + n]

    def view(self, start, n):
        """Any sub-range of the arena as an operand (aliases and partial overlaps)."""
        return self.dev[start:start + n]

    def download(self, ctx):
        ctx.synchronize()
        self.host = bits(self.dev.detach().cpu().numpy()).copy()
        return self

    # ---- checks on the last download (or on self.host, which a CPU test edits) ----------------
    def get(self, name):
        s, n, _ = self.ops[name]
        return self.host[s:s + n].view(np.float64).copy()

    def _body_mask(self, outputs):
        m = np.zeros(self.size, bool)
        for s, n, out in self.ops.values():
            if out == outputs:
                m[s:s + n] = True
        return m

    def check(self):
        """Arena indices of the guard words (everything outside the operand bodies) that changed."""
        guard = ~(self._body_mask(True) | self._body_mask(False))
        return np.flatnonzero(guard & (self.host != self.image))

    def inputs_changed(self):
        return np.flatnonzero(self._body_mask(False) & (self.host != self.image))

    def changed(self):
        """Every arena index that changed, output bodies included (a rejected call: none)."""
        return np.flatnonzero(self.host != self.image)

    def untouched(self, name, lo=0, hi=None):
        s, n, _ = self.ops[name]
        hi = n if hi is None else hi
        return bool(np.array_equal(self.host[s + lo:s + hi], self.image[s + lo:s + hi]))

    def owner(self, idx):
        """The operand whose body or guard holds arena index idx (for messages)."""
        for name, (s, n, _) in self.ops.items():
            if s - self.guard <= idx < s + n + self.guard:
                return name, int(idx) - s
        return None, int(idx)
