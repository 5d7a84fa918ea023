"""Shared by the top-level rebuild's tests (tests/test_world_rebuild_host.py, tests/test_gpu_world_rebuild.py): the rule of
rayaccel_amd/csrc/racc_world_rebuild_rule.h restated in numpy, a walk of a top-level tree, and the worlds that stress its height."""
import numpy as np

from world_helpers import IDENTITY

LEAF = 1 << 24
INNER = 0x80000000


def height_bound(count, disabled_possible=False):
    """Rule 8: a record's split bit is below its parent's, and only the 30 field bits, the low ceil(log2(count)) index bits and — on the
    device — the disabled bit can differ between two keys; never more than the count - 1 records there are."""
    by_bits = 30 + int(disabled_possible) + int(np.ceil(np.log2(count))) if count > 1 else 30 + int(disabled_possible)
    return min(by_bits, max(count - 1, 1))


def numpy_keys(world_boxes):
    """Rules 2-5 in numpy.float64: the sorted 64-bit keys of the instances with these world boxes."""
    b = np.asarray(world_boxes, np.float32).astype(np.float64)
    c = (0.5 * b[:, :3] + 0.5 * b[:, 3:]).astype(np.float32)
    lo, hi = c.min(0), c.max(0)
    field = np.zeros(len(c), np.uint64)
    for axis in range(3):
        if not hi[axis] > lo[axis]:
            continue
        v = (c[:, axis].astype(np.float64) - np.float64(lo[axis])) / (np.float64(hi[axis]) - np.float64(lo[axis])) * 1024.0
        q = np.minimum(np.floor(v), 1023.0).astype(np.uint64)
        for bit in range(10):
            field |= ((q >> np.uint64(bit)) & np.uint64(1)) << np.uint64(3 * bit + 2 - axis)
    return np.sort((field << np.uint64(32)) | np.arange(len(c), dtype=np.uint64))


def numpy_lbvh(world_boxes):
    """Rules 2-6: (first [records], last [records], order [count]) — every range split behind the last position that shares with its
    first key more leading bits than its last key does, by a scan over the range."""
    keys = numpy_keys(world_boxes)
    n = len(keys)
    order = (keys & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    first, last = np.zeros(max(n - 1, 1), np.uint32), np.zeros(max(n - 1, 1), np.uint32)
    if n == 1:
        first[0] = LEAF
        return first, last, order
    todo = [(0, 0, n - 1)]
    while todo:
        record, a, b = todo.pop()
        x = keys[a:b] ^ keys[a]                                      # positions a .. b - 1 against key[a]
        differ = int(keys[a] ^ keys[b]).bit_length()                 # the highest differing bit of the two ends, plus one
        s = a + int(np.nonzero(x < np.uint64(1 << (differ - 1)))[0].max())      # shares more: differs only below that bit
        for side, (ca, cb, child) in enumerate(((a, s, s), (s + 1, b, s + 1))):
            ref = LEAF | ca if ca == cb else INNER | child
            (last if side else first)[record] = ref
            if ca != cb:
                todo.append((child, ca, cb))
    return first, last, order


def walk_height(first, last, count):
    """Levels of records on the longest root path; asserts that every record is reached once and every position named once."""
    seen_records, seen_positions = np.zeros(len(first), int), np.zeros(count, int)
    height, todo = 0, [(0, 1)]
    seen_records[0] = 1
    while todo:
        record, depth = todo.pop()
        height = max(height, depth)
        for ref in (int(first[record]), int(last[record])):
            if ref & INNER:
                child = ref & 0x7FFFFFFF
                assert 0 < child < len(first), "child index out of range"
                seen_records[child] += 1
                todo.append((child, depth + 1))
            elif ref >> 24:
                assert ref >> 24 == 1 and (ref & 0xFFFFFF) < count
                seen_positions[ref & 0xFFFFFF] += 1
            else:
                assert count == 1 and ref == 0, "an empty reference outside a one-instance world"
    assert (seen_records == 1).all(), "a record is reached twice or never"
    assert (seen_positions == 1).all(), "a position of order is in no leaf or in several"
    return height


def translated(offsets):
    """[N,3,4] identity transforms translated by `offsets` [N,3]."""
    t = np.tile(IDENTITY, (len(offsets), 1, 1))
    t[:, :, 3] = np.asarray(offsets, np.float32)
    return t


def common_centre_world(count=1000):
    """`count` instances in one place: every Morton field is equal, the index bits alone decide."""
    return translated(np.tile(np.float32([3.0, -2.0, 5.0]), (count, 1)))


def chain_world(length, extra_at_the_end=0):
    """31 instances whose centres lie at length * 2^-k, k = 0 .. 30, on the x axis — every split of the Morton field cuts one instance
    off the rest — and `extra_at_the_end` more on top of the last one."""
    x = [length * 2.0 ** -k for k in range(31)] + [length * 2.0 ** -30] * extra_at_the_end
    offsets = np.zeros((len(x), 3), np.float32)
    offsets[:, 0] = x
    return translated(offsets)
