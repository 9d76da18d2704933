"""The CPU restatement of the tree builder (bvh_restatement.py) held to constructions that share no code with it: Karras' bottom-up topology against a
top-down builder, the dynamic programme and its replay against the exhaustive enumeration of every collapse, and the node count of a cloud of identical
gaussians. No GPU: test_hip_bvh_build.py holds the kernels to the restatement, this file holds the restatement."""
import time

import numpy as np
import pytest

import bvh_restatement as br

SIZES = [2, 3, 8, 9, 64, 65, 255, 256, 257, 1000]


def key_set(kind, n, rng):
    if kind == "distinct":
        keys = rng.choice(1 << 20, size=n, replace=False).astype(np.uint64) << np.uint64(int(rng.integers(0, 43)))
    elif kind == "runs":  # runs of duplicates of random length (most keys repeat)
        keys = rng.integers(0, max(n // 4, 1), size=n).astype(np.uint64) << np.uint64(int(rng.integers(0, 50)))
    elif kind == "equal":
        keys = np.full(n, 0x1249249249249249, np.uint64)
    else:
        raise KeyError(kind)
    return np.sort(keys)


def top_down(keys):
    """{(first, last): ((first, split), (split + 1, last))} of the builder that splits a range at the highest differing bit of the augmented key
    (key << 32) | index - distinct for every index, so every range of two or more splits."""
    aug = [(int(k) << 32) | i for i, k in enumerate(keys)]
    out, stack = {}, [(0, len(aug) - 1)]
    while stack:
        a, b = stack.pop()
        if a == b:
            continue
        bit = (aug[a] ^ aug[b]).bit_length() - 1  # sorted: the highest bit in which first and last differ is 0 at `a` and 1 at `b`
        split = a
        while not (aug[split + 1] >> bit) & 1:
            split += 1
        out[(a, b)] = ((a, split), (split + 1, b))
        stack += [(a, split), (split + 1, b)]
    return out


@pytest.mark.parametrize("kind", ["distinct", "runs", "equal"])
@pytest.mark.parametrize("n", SIZES)
def test_karras_equals_the_top_down_builder(n, kind):
    keys = key_set(kind, n, np.random.default_rng(n))
    if kind == "distinct":
        assert len(np.unique(keys)) == n
    if kind == "runs" and n >= 64:
        assert len(np.unique(keys)) < n // 2
    left, right, first, last = br.karras(keys)
    ref = top_down(keys)

    def rng_of(c):
        return (c - (n - 1),) * 2 if c >= n - 1 else (int(first[c]), int(last[c]))

    got = {(int(first[i]), int(last[i])): (rng_of(int(left[i])), rng_of(int(right[i]))) for i in range(n - 1)}
    assert len(got) == n - 1  # every internal node has a range of its own
    assert got == ref
    assert (int(first[0]), int(last[0])) == (0, n - 1)


# ------------------------------------------------------------------------------------------------ the programme
def random_tree(n, rng):
    """A random binary tree over n leaves in the builder's id space (internal ids in pre-order, root 0)."""
    left, right = np.zeros(n - 1, np.int64), np.zeros(n - 1, np.int64)
    counter = [0]

    def build(a, b):
        if a == b:
            return (n - 1) + a
        i = counter[0]
        counter[0] += 1
        s = int(rng.integers(a, b))
        left[i] = build(a, s)
        right[i] = build(s + 1, b)
        return i

    build(0, n - 1)
    return left, right


def random_boxes(n, rng, empty_share=0.0):
    c = rng.uniform(-1, 1, (n, 3))
    e = rng.uniform(0.01, 0.3, (n, 3))
    box = np.concatenate([c - e, c + e], axis=1).astype(np.float32)
    box[rng.uniform(size=n) < empty_share] = np.array([3.0e38] * 3 + [-3.0e38] * 3, np.float32)
    return box


def enumerated_minimum(left, right, area):
    """Least sum of wide-node areas over EVERY collapse: a wide node stands for a binary internal node and its children are a cut of that node's subtree
    below it (every leaf under the node has exactly one member of the cut on its path) of at most 8 members; internal members are wide nodes themselves."""
    nb = len(left)

    def cuts(c):  # every cut of the subtree of c, c itself included
        if c >= nb:
            return [[c]]
        return [[c]] + [a + b for a in cuts(int(left[c])) for b in cuts(int(right[c])) if len(a) + len(b) <= br.WIDTH]

    memo = {}

    def cost(b):
        if b >= nb:
            return 0.0
        if b not in memo:
            below = [x + y for x in cuts(int(left[b])) for y in cuts(int(right[b])) if len(x) + len(y) <= br.WIDTH]
            memo[b] = area[b] + min(sum(cost(c) for c in cut) for cut in below)
        return memo[b]

    return cost(0)


def leaves_under(left, right, c):
    nb = len(left)
    return [c - nb] if c >= nb else leaves_under(left, right, int(left[c])) + leaves_under(left, right, int(right[c]))


def check_replay(left, right, T, area):
    levels = br.replay(left, right, T)
    nb = len(left)
    assert [b for b, _ in levels[0]] == [0]
    for d, level in enumerate(levels):
        for b, child in level:
            assert 2 <= len(child) <= br.WIDTH
            pos = [leaves_under(left, right, c) for c in child]
            flat = [p for ps in pos for p in ps]
            assert flat == sorted(leaves_under(left, right, b)) and flat == list(range(flat[0], flat[-1] + 1))  # a cut, in ascending leaf order
            inner = [c for c in child if c < nb]
            if inner:
                assert set(inner) <= {b2 for b2, _ in levels[d + 1]}
        assert d == 0 or sorted(b for b, _ in level) == sorted(c for _, ch in levels[d - 1] for c in ch if c < nb)
    return levels, br.replay_cost(levels, area)


@pytest.mark.parametrize("n", [2, 3, 4, 5, 6, 7, 8, 9])
def test_programme_and_replay_equal_the_enumerated_minimum(n):
    rng = np.random.default_rng(100 + n)
    for trial in range(12):
        if trial % 3 == 2:
            keys = key_set("runs" if trial % 2 else "distinct", n, rng)
            left, right, _, _ = br.karras(keys)
        else:
            left, right = random_tree(n, rng)
        boxes = random_boxes(n, rng, empty_share=0.3 if trial % 4 == 3 else 0.0)
        box, area, T, h = br.sah_rows(left, right, boxes)
        best = enumerated_minimum(left, right, area)
        assert T[0, 1] == pytest.approx(best, rel=1e-13, abs=0.0)
        _, c = check_replay(left, right, T, area)
        assert c == pytest.approx(T[0, 1], rel=1e-13, abs=0.0)
        assert np.all(np.diff(T[:, 1:], axis=1) <= 0)  # more slots never cost more
        assert 1 <= h <= n - 1


def test_rows_of_empty_boxes():
    """A subtree of unusable gaussians only: its box stays empty (lo > hi), its area and rows are 0, and it is neutral in its parent's box."""
    left, right = np.array([1, 3, 5]), np.array([2, 4, 6])  # 4 leaves: root 0 = (1, 2), node 1 = leaves 0, 1, node 2 = leaves 2, 3
    boxes = random_boxes(4, np.random.default_rng(0))
    boxes[:2] = np.array([3.0e38] * 3 + [-3.0e38] * 3, np.float32)
    box, area, T, h = br.sah_rows(left, right, boxes)
    assert h == 2 and area[1] == 0 and np.all(T[1] == 0) and box[1, 0] > box[1, 3]
    assert np.array_equal(box[0], box[2]) and area[0] == area[2] > 0


@pytest.mark.parametrize("n,levels_expected", [(64, [1, 8]), (100, [1, 2, 12]), (512, [1, 8, 64])])
def test_identical_gaussians_collapse_to_the_flattest_tree(n, levels_expected):
    """Equal keys, equal boxes of area A > 0: every wide node costs A, so the optimum is the least number of nodes, ceil((n - 1) / 7) (a node with 8
    children removes 7 of the n - 1 binary nodes). The level sizes are what dp_distribute's tie-break (the first k that attains the minimum) gives; at
    n = 100 other splits of the 15 nodes over the levels cost the same. The box's area and its multiples are exact, so ties are exact ties."""
    keys = key_set("equal", n, None)
    left, right, _, _ = br.karras(keys)
    boxes = np.tile(np.array([[-0.5, -0.5, -0.5, 0.5, 0.5, 0.5]], np.float32), (n, 1))
    _, area, T, _ = br.sah_rows(left, right, boxes)
    assert area[0] == 3.0
    levels, cost = check_replay(left, right, T, area)
    assert sum(len(level) for level in levels) == -(-(n - 1) // 7)
    assert cost == T[0, 1] == 3.0 * -(-(n - 1) // 7)
    assert [len(level) for level in levels] == levels_expected


def test_restatement_is_quick_at_the_largest_gpu_size():
    rng = np.random.default_rng(7)
    keys = np.sort(rng.integers(0, 1 << 62, 4096).astype(np.uint64))
    t0 = time.perf_counter()
    left, right, _, _ = br.karras(keys)
    _, area, T, _ = br.sah_rows(left, right, random_boxes(4096, rng))
    levels = br.replay(left, right, T)
    dt = time.perf_counter() - t0
    assert sum(len(level) for level in levels) < 4095
    assert dt < 5.0, dt  # (measured 0.25 - 0.5 s; the bar only catches a quadratic slip)


# ------------------------------------------------------------------------------------------------ keys
def test_morton_keys_known_answers():
    frame = np.array([0, 0, 0, 65536, 65536, 65536], np.float32)  # u = v: q = trunc(v * 2^21)
    mean = np.array([[0, 0, 0], [0.5, 0, 0], [0, 0.5, 0], [0, 0, 0.5], [2.0 ** -21, 0, 0], [1.0, 1.0, 1.0], [-1.0, 2.0, np.nan], [np.inf, -np.inf, 0.25],
                     [(2.0 ** 21 - 1) / 2.0 ** 21, 0, 0]], np.float32)
    keys = br.morton_keys(mean, frame)
    top = 1 << 62
    every_third = sum(1 << (3 * i) for i in range(21))
    expected = [0, top, top >> 1, top >> 2, 4, (1 << 63) - 1, every_third << 1, 1 << 57, every_third << 2]
    assert [int(k) for k in keys] == expected


def test_morton_keys_interleave_every_bit():
    rng = np.random.default_rng(3)
    q = rng.integers(0, 1 << 21, (500, 3))
    mean = (q.astype(np.float64) / 2.0 ** 21).astype(np.float32)  # exact: 21 bits
    keys = br.morton_keys(mean, np.array([0, 0, 0, 65536, 65536, 65536], np.float32))
    for k, (x, y, z) in zip(keys, q):
        ref = 0
        for i in range(21):
            ref |= ((int(x) >> i) & 1) << (3 * i + 2) | ((int(y) >> i) & 1) << (3 * i + 1) | ((int(z) >> i) & 1) << (3 * i)
        assert int(k) == ref


def test_wide_tree_reader_and_canonical_form():
    """Two numberings of one hand-made tree over 10 leaves read to the same canonical form; a repeated leaf raises."""
    E, L = br.EMPTY_SLOT, br.LEAF_FLAG

    def nodes_of(links):
        w = np.zeros((len(links), 8, 4), np.uint32)
        for i, row in enumerate(links):
            w[i, :, 3] = row + [E] * (8 - len(row))
        return w

    a = nodes_of([[1, L | 4, 2], [L | 0, L | 1, L | 2, L | 3], [L | 5, L | 6, L | 7, L | 8, L | 9]])
    b = nodes_of([[2, L | 4, 1], [L | 5, L | 6, L | 7, L | 8, L | 9], [L | 0, L | 1, L | 2, L | 3]])
    ta, tb = br.wide_tree_from_links(a, 10), br.wide_tree_from_links(b, 10)
    assert ta[0]["range"] == (0, 9) and ta[0]["leaves"] == 10 and ta[2]["depth"] == 1
    assert [(s[1], s[2]) for s in ta[0]["slots"]] == [(0, 3), (4, 4), (5, 9)]
    assert br.canonical_form(ta) == br.canonical_form(tb) == [[((0, 3), (4, 4), (5, 9))], sorted([((0, 0), (1, 1), (2, 2), (3, 3)), ((5, 5), (6, 6), (7, 7), (8, 8), (9, 9))])]
    with pytest.raises(ValueError):
        br.wide_tree_from_links(nodes_of([[L | 0, L | 0]]), 2)
