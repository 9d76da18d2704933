"""The tree builder of csrc/bvh.hip restated for the CPU, stage by stage: Morton keys (k_morton), Karras topology (k_karras), the SAH dynamic programme
(k_sah_bottom_up), its top-down replay (k_collapse_level), and a reader of the wide tree that Raytracer.debug_tree() exports. numpy and plain Python; fp64
unless stated. The frame comes from drift_scenes.frame_restated (CPU) or from Raytracer.debug_bvh_state (GPU tests). test_bvh_restatement_host.py checks
this file against independent constructions (a top-down builder, exhaustive enumeration of collapses); test_hip_bvh_build.py holds the kernels to it.
A plain module: no fixtures, nothing is collected from here.

Id space of the binary tree over n sorted leaves (the kernel's): internal node i in [0, n-2] -> i, leaf at sorted position j -> (n-1) + j; root = 0."""
import numpy as np

from drift_scenes import frame_restated  # noqa: F401  (re-exported: the frame rule belongs to the builder)

WIDTH = 8
LEAF_FLAG = 0x80000000
EMPTY_SLOT = 0xFFFFFFFF


# ------------------------------------------------------------------------------------------------ keys
def _spread21(v):
    """Bit i of the 21-bit v moves to bit 3i (uint64), one bit at a time: the reference for spread21's five masks."""
    v = v.astype(np.uint64)
    out = np.zeros_like(v)
    for i in range(21):
        out |= ((v >> np.uint64(i)) & np.uint64(1)) << np.uint64(3 * i)
    return out


def morton_keys(mean_f32, frame_f32):
    """uint64 [n] keys of k_morton, bit for bit. Per axis, in fp32: q = uint32(clip(((v - o) * s) * 2^-16 * 2^21, 0, 2^21 - 1)), truncated; a non-finite
    coordinate gives 0; key = x, y, z bits interleaved, x highest. No product is followed by a sum, so there is no multiply-add a compiler could contract,
    and both power-of-two factors are exact: the fp32 value is the same on every IEEE machine."""
    m = np.asarray(mean_f32, np.float32).reshape(-1, 3)
    fr = np.asarray(frame_f32, np.float32)
    o, s = fr[:3], fr[3:]
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        u = ((m - o) * s) * np.float32(1.0 / 65536.0)
        u = np.where(np.isfinite(m), u, np.float32(0.0)).astype(np.float32)
        t = np.minimum(np.maximum(u * np.float32(2097152.0), np.float32(0.0)), np.float32(2097151.0))  # fmaxf, then fminf
    q = t.astype(np.uint32)  # truncation (the values are in [0, 2^21 - 1])
    return (_spread21(q[:, 0]) << np.uint64(2)) | (_spread21(q[:, 1]) << np.uint64(1)) | _spread21(q[:, 2])


# ------------------------------------------------------------------------------------------------ topology
def karras(sorted_keys):
    """(left, right, first, last): int64 [n-1] arrays of Karras 2012 over the sorted keys, as k_karras builds them. delta(i, j) = number of leading
    bits key i and key j share (64-bit count), for equal keys 64 + clz32(i ^ j), -1 outside [0, n)."""
    keys = [int(k) for k in np.asarray(sorted_keys).reshape(-1)]
    n = len(keys)

    def delta(i, j):
        if j < 0 or j >= n:
            return -1
        a, b = keys[i], keys[j]
        if a == b:
            return 64 + 32 - (i ^ j).bit_length()
        return 64 - (a ^ b).bit_length()

    left, right = np.zeros(max(n - 1, 0), np.int64), np.zeros(max(n - 1, 0), np.int64)
    first, last = np.zeros(max(n - 1, 0), np.int64), np.zeros(max(n - 1, 0), np.int64)
    for i in range(n - 1):
        d = 1 if delta(i, i + 1) - delta(i, i - 1) >= 0 else -1
        dmin = delta(i, i - d)
        lmax = 2
        while delta(i, i + lmax * d) > dmin:
            lmax *= 2
        length, t = 0, lmax // 2
        while t >= 1:
            if delta(i, i + (length + t) * d) > dmin:
                length += t
            t //= 2
        j = i + length * d
        dnode = delta(i, j)
        s, t = 0, length
        while True:
            t = (t + 1) // 2
            if delta(i, i + (s + t) * d) > dnode:
                s += t
            if t <= 1:
                break
        gamma = i + s * d + min(d, 0)
        lo, hi = min(i, j), max(i, j)
        left[i] = (n - 1) + gamma if lo == gamma else gamma
        right[i] = (n - 1) + gamma + 1 if hi == gamma + 1 else gamma + 1
        first[i], last[i] = lo, hi
    return left, right, first, last


def bottom_up_order(left, right):
    """Internal ids, children before parents (reverse of a pre-order from the root)."""
    nb = len(left)
    order, stack = [], [0] if nb else []
    while stack:
        i = stack.pop()
        order.append(i)
        for c in (int(left[i]), int(right[i])):
            if c < nb:
                stack.append(c)
    return order[::-1]


# ------------------------------------------------------------------------------------------------ the programme
def _distribute(Tl, Tr, j):
    """(D(n, j), the first k in 1..j-1 that attains it): D = min over k of T(left, min(k, 7)) + T(right, min(j - k, 7)); row index 0 unused."""
    best, best_k = float("inf"), 1
    for k in range(1, j):
        c = Tl[min(k, 7)] + Tr[min(j - k, 7)]
        if c < best:
            best, best_k = c, k
    return best, best_k


_ZERO_ROW = [0.0] * 8


def sah_rows(left, right, leaf_boxes_f32):
    """(box [n-1,6], area [n-1], T [n-1,8], h): the rows of the comment block above k_sah_bottom_up in fp64. leaf_boxes_f32 [n,6] (lo xyz, hi xyz) by SORTED
    POSITION; an empty leaf box has lo > hi (the builder stores 3e38 / -3e38) and is neutral in the union by min / max alone. area = half the surface area,
    0 for a node of empty boxes only (lo.x > hi.x). T[:, 0] = 0 (unused), T[:, i] = T(node, i):
        leaf: T = 0;  T(n, 1) = area(n) + D(n, 8);  T(n, i) = min(D(n, i), T(n, i - 1)), i = 2..7.
    h = height of the binary tree in internal nodes (a node over two leaves has height 1)."""
    nb = len(left)
    n = nb + 1
    lb = np.asarray(leaf_boxes_f32, np.float64).reshape(n, 6)
    box, area = np.zeros((nb, 6)), np.zeros(nb)
    rows = [None] * nb
    height = [0] * nb
    for i in bottom_up_order(left, right):
        ch = (int(left[i]), int(right[i]))
        bs = [lb[c - nb] if c >= nb else box[c] for c in ch]
        box[i, :3] = np.minimum(bs[0][:3], bs[1][:3])
        box[i, 3:] = np.maximum(bs[0][3:], bs[1][3:])
        if box[i, 0] <= box[i, 3]:
            dx, dy, dz = (max(float(box[i, 3 + a] - box[i, a]), 0.0) for a in range(3))
            area[i] = dx * dy + dy * dz + dz * dx
        Tl, Tr = (_ZERO_ROW if c >= nb else rows[c] for c in ch)
        T = [0.0] * 8
        T[1] = area[i] + _distribute(Tl, Tr, 8)[0]
        for k in range(2, 8):
            T[k] = min(_distribute(Tl, Tr, k)[0], T[k - 1])
        rows[i] = T
        height[i] = 1 + max(0 if c >= nb else height[c] for c in ch)
    return box, area, np.array(rows, np.float64).reshape(nb, 8), (height[0] if nb else 0)


def replay(left, right, T):
    """The wide tree the programme's decisions produce (k_collapse_level): a list of levels, each a list of (binary id of the wide node, [child ids in
    slot order]); a child id >= n-1 is a leaf, any other id is a wide node of the next level. Every entry carries the slots the optimum grants it; an internal
    entry with b > 1 slots dissolves into its two children with the split that attains D(node, b') for the largest b' <= b with D(node, b') <= T(node, b' - 1)
    (at equal cost the flatter tree wins), and stays a wide node of its own when there is none."""
    nb = len(left)
    T = np.asarray(T, np.float64)

    def row(c):
        return _ZERO_ROW if c >= nb else [float(x) for x in T[c]]

    levels, frontier = [], [0] if nb else []
    while frontier:
        level, nxt = [], []
        for bnode in frontier:
            child = [int(left[bnode]), int(right[bnode])]
            k = _distribute(row(child[0]), row(child[1]), WIDTH)[1]
            budget = [k, WIDTH - k]
            at = 0
            while at < len(child):
                c = child[at]
                if c >= nb:
                    at += 1
                    continue
                Tc, Tl, Tr = row(c), row(int(left[c])), row(int(right[c]))
                b, k = min(budget[at], 7), 1
                while b >= 2:
                    d, k = _distribute(Tl, Tr, b)
                    if d <= Tc[b - 1]:
                        break
                    b -= 1
                if b < 2:
                    budget[at] = 1
                    at += 1
                    continue
                child[at:at + 1] = [int(left[c]), int(right[c])]
                budget[at:at + 1] = [k, b - k]
            assert len(child) <= WIDTH
            level.append((bnode, child))
            nxt.extend(c for c in child if c < nb)
        levels.append(level)
        frontier = nxt
    return levels


def replay_cost(levels, area):
    return float(sum(area[b] for level in levels for b, _ in level))


# ------------------------------------------------------------------------------------------------ the exported wide tree
def unpack_slots(wnodes):
    """(lo [nw,8,3], hi [nw,8,3], link [nw,8]) of exported wide nodes (uint32 [nw,8,4]): 16-bit cells lo.x | lo.y << 16, lo.z | hi.x << 16, hi.y | hi.z << 16."""
    w = np.asarray(wnodes).view(np.uint32).reshape(-1, WIDTH, 4).astype(np.int64)
    lo = np.stack([w[..., 0] & 0xFFFF, w[..., 0] >> 16, w[..., 1] & 0xFFFF], axis=-1)
    hi = np.stack([w[..., 1] >> 16, w[..., 2] & 0xFFFF, w[..., 2] >> 16], axis=-1)
    return lo, hi, w[..., 3]


def wide_tree_from_links(wnodes, n):
    """Per wide node of an exported tree, reached from node 0: a dict {depth, slots, range, leaves} with slots = [(slot index, first position, last position,
    number of leaves below, link)] for the used slots in slot order, range = (first, last) over all slots and leaves = their number. Raises on a node or a
    leaf reached twice and on a link out of range (check_bvh's own ground; restated here so that a bad export cannot loop)."""
    _, _, link = unpack_slots(wnodes)
    nw = link.shape[0]
    depth, order, seen = {0: 0}, [0], {0}
    for w in order:  # breadth first
        for k in range(WIDTH):
            l = int(link[w, k])
            if l == EMPTY_SLOT or l & LEAF_FLAG:
                continue
            if l >= nw or l in seen:
                raise ValueError(f"wide node {w} slot {k}: bad or repeated child {l}")
            seen.add(l)
            depth[l] = depth[w] + 1
            order.append(l)
    nodes = {}
    leaf_seen = np.zeros(n, bool)
    for w in reversed(order):
        slots = []
        for k in range(WIDTH):
            l = int(link[w, k])
            if l == EMPTY_SLOT:
                continue
            if l & LEAF_FLAG:
                p = l & ~LEAF_FLAG
                if p >= n or leaf_seen[p]:
                    raise ValueError(f"wide node {w} slot {k}: bad or repeated leaf {p}")
                leaf_seen[p] = True
                slots.append((k, p, p, 1, l))
            else:
                c = nodes[l]
                slots.append((k, c["range"][0], c["range"][1], c["leaves"], l))
        nodes[w] = dict(depth=depth[w], slots=slots, range=(min(s[1] for s in slots), max(s[2] for s in slots)) if slots else (0, -1),
                        leaves=sum(s[3] for s in slots))
    return nodes


def canonical_form(nodes):
    """Per level, the sorted list of the nodes' slot ranges: equal for two trees that differ in the numbering of the nodes inside a level only."""
    levels = {}
    for nd in nodes.values():
        levels.setdefault(nd["depth"], []).append(tuple((s[1], s[2]) for s in nd["slots"]))
    return [sorted(levels[d]) for d in sorted(levels)]
