"""tests/vector_contract_cases.py can fail: the arena reports exactly the guard word a
one-double overrun changes, the range predicate equals brute force, and the restated
amg_vector_read partials add up to the plain sum.  No GPU."""
import numpy as np
import pytest

from tests import vector_contract_cases as V


def _arena():
    a = V.Arena()
    a.input("x", np.arange(1.0, 6.0), 1)
    a.output("y", 7, 7)
    a.output("z", 4, 2, init=np.full(4, 2.5))
    a.build_image()
    return a


def test_layout_and_fill():
    a = _arena()
    sx, sy, sz = a.start("x"), a.start("y"), a.start("z")
    assert (sx % 8, sy % 8, sz % 8) == (1, 7, 2)
    assert sx >= V.G and sy - (sx + 5) >= 2 * V.G and sz - (sy + 7) >= 2 * V.G
    assert a.size == sz + 4 + V.G
    img = a.image
    assert np.all(img[sx - V.G:sx] == V.NAN_BITS) and np.all(img[sx + 5:sx + 5 + V.G] == V.NAN_BITS)
    assert np.array_equal(a.get("x"), np.arange(1.0, 6.0)) and np.array_equal(a.get("z"), np.full(4, 2.5))
    # canaries: NaN as doubles, distinct per index, their payload is the index
    c = img[sy - V.G:sy + 7 + V.G]
    assert np.all(np.isnan(c.view(np.float64))) and np.unique(c).size == c.size
    assert np.array_equal(c & np.uint64(0xFFFFFFFFFF), np.arange(sy - V.G, sy + 7 + V.G).astype(np.uint64))
    assert a.check().size == 0 and a.inputs_changed().size == 0 and a.changed().size == 0
    assert a.untouched("y") and a.untouched("z")


@pytest.mark.parametrize("name", ["x", "y", "z"])
@pytest.mark.parametrize("where", ["past", "before"])
def test_one_double_overrun_is_reported_exactly(name, where):
    a = _arena()
    s, n, _ = a.ops[name]
    i = s + n if where == "past" else s - 1
    a.host[i] = V.bits(np.array([3.0]))[0]
    assert a.check().tolist() == [i]
    assert a.owner(i) == (name, n if where == "past" else -1)
    assert a.inputs_changed().size == 0


def test_shifted_and_duplicated_stores_are_reported():
    a = _arena()
    s, n, _ = a.ops["y"]
    a.host[s + n] = a.image[s + n - 1]  # the neighbouring canary, duplicated one word on
    assert a.check().tolist() == [s + n]
    a = _arena()
    sx = a.start("x")
    a.host[sx - 1] = V.canary(sx - 1)   # a canary written into an input's NaN guard
    assert a.check().tolist() == [sx - 1]


def test_body_changes_are_told_apart():
    a = _arena()
    sx, sy = a.start("x"), a.start("y")
    a.host[sx + 2] = V.bits(np.array([-0.0]))[0]
    assert a.inputs_changed().tolist() == [sx + 2] and a.check().size == 0
    a.host[sy + 3] = V.bits(np.array([1.0]))[0]
    assert not a.untouched("y") and a.untouched("y", 0, 3) and a.untouched("y", 4)
    assert a.check().size == 0 and sorted(a.changed().tolist()) == [sx + 2, sy + 3]


def test_overlaps_equals_brute_force():
    for a0 in range(0, 7):
        for na in range(0, 5):
            for b0 in range(0, 7):
                for nb in range(0, 5):
                    brute = bool(set(range(a0, a0 + na)) & set(range(b0, b0 + nb)))
                    assert V.overlaps(a0, na, b0, nb) == brute, (a0, na, b0, nb)
                    assert V.overlaps(b0, nb, a0, na) == brute


@pytest.mark.parametrize("n", V.COPY_SIZES)
def test_read_partials_sum_to_the_plain_sum(n):
    src = V.read_data(n)
    want = V.read_partials_expected(src)
    assert want.size == V.read_partial_count(n) == 4 * max(1, -(-(n // 2) // 1024))
    assert want.sum() == src[:2 * (n // 2)].sum()
    assert np.all(np.isfinite(want))  # the NaN tail of an odd n is in no pair
    if n >= 2:
        # one changed element moves exactly its slot: pair p of workgroup b, wave (p % 256) // 64
        k = 2 * ((n // 2) - 1)
        src2 = src.copy()
        src2[k] += 1.0
        p = k // 2
        d = np.flatnonzero(V.read_partials_expected(src2) != want)
        assert d.tolist() == [4 * (p // 1024) + ((p % 1024) % 256) // 64]


def test_read_partials_slot_rule_by_hand():
    # 1024 pairs + 65: workgroup 0 full (256 pairs per wave), workgroup 1 holds pairs 0..64:
    # wave 0 gets 64, wave 1 gets one, waves 2 and 3 none
    n = 2 * (1024 + 65)
    got = V.read_partials_expected(np.ones(n))
    assert got.tolist() == [512.0] * 4 + [128.0, 2.0, 0.0, 0.0]
