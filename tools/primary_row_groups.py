"""CPU estimate (pure numpy, no GPU) of what the backward chain's primary hit rows look like to the row sum of trace.hip
(primary_table_add): per hit row of an 8x8 tile (lane = 8 y + x) the active lanes, the distinct gaussians among them (= the leaders
of the row), the pointer-jumping steps the group sums need (ceil(log2(largest group))), and - what the table update cost until round 21
and what was measured against it (profiles/HISTORY.md) - the lanes left after two DPP pre-sum levels (lane ^ 1, then lane ^ 8), the
serialised claim-word rounds of those lanes (= the largest number of them that hold the same gaussian) and the steps behind the levels.

    python tools/primary_row_groups.py [--gaussians 1000000] [--variant init] [--tiles 60] [--seed 0]

The scene is synthetic.make_scene, the camera synthetic.default_camera at 1920x1080, jitter off. A ray's hits are restated, not traced:
a gaussian is a candidate where the ray's closest-approach point lies inside its ellipsoid (semi-axes exp(scale) x scaling factor) in
front of the camera, its alpha is MAX_ALPHA x opacity x exp(-|x|^6 / 6) at that point (exp_power 3), candidates below alpha_threshold
0.005 are dropped, and the list is composited front to back until the transmittance falls below 0.01. Row i of a tile holds the i-th hit
of each of its rays; the backward walks the rows far to near, which no per-row figure depends on."""
import argparse
import importlib
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
syn = importlib.import_module("editable-gaussian-reflections_amd.synthetic")

MAX_ALPHA, ALPHA_THRESHOLD, T_THRESHOLD, EXP_POWER = 0.9999, 0.005, 0.01, 3.0


def tile_rays(cam, W, H, tx, ty):
    """Unit directions [64, 3] of the 8x8 tile (tx, ty), lane = 8 y + x, through the pixel centres."""
    view = math.tan(float(cam["fov"]) * 0.5)
    px, py = np.meshgrid(np.arange(8) + 8 * tx, np.arange(8) + 8 * ty, indexing="xy")  # [y, x]
    x = (W / H) * view * (2.0 * ((px.ravel() + 0.5) / W) - 1.0)
    y = view * (1.0 - 2.0 * ((py.ravel() + 0.5) / H))
    d = np.stack([x, y, -np.ones_like(x)], -1) @ cam["c2w"].astype(np.float64).T
    return d / np.linalg.norm(d, axis=-1, keepdims=True)


def tile_rows(g, cam, W, H, tx, ty, pre):
    """pos [rows, 64] int64 (-1: the lane's ray has no hit in this row) of one tile. `pre`: per-gaussian constants."""
    mean, Wm, opacity, sf, rmax = pre
    o = cam["origin"].astype(np.float64)
    d = tile_rays(cam, W, H, tx, ty)
    dc = d.mean(0)
    dc /= np.linalg.norm(dc)
    half = np.arccos(np.clip((d @ dc).min(), -1.0, 1.0))  # the tile's cone around its mean direction
    rel = mean - o
    dist = np.linalg.norm(rel, axis=1)
    ang = np.arccos(np.clip((rel @ dc) / dist, -1.0, 1.0))
    near = np.nonzero(ang <= half + np.arcsin(np.clip(rmax / dist, 0.0, 1.0)) + 1e-6)[0]  # every gaussian a ray of the tile can meet
    Wn = Wm[near]                                        # [n, 3, 3]: world -> unit-sphere object space
    lo = np.einsum("nij,nj->ni", Wn, o - mean[near])     # [n, 3]
    ld = np.einsum("nij,rj->rni", Wn, d)                 # [64, n, 3]
    norm = np.linalg.norm(ld, axis=-1)
    dhat = ld / norm[..., None]
    tl = -(lo[None] * dhat).sum(-1)
    u = lo[None] + tl[..., None] * dhat                  # closest approach
    t = tl / norm
    sq = ((u * sf[near][None, :, None]) ** 2).sum(-1)
    alpha = MAX_ALPHA * opacity[near][None] * np.exp(-(sq ** EXP_POWER) / (2.0 * EXP_POWER))
    cand = ((u * u).sum(-1) <= 1.0) & (tl > 0.0) & (alpha >= ALPHA_THRESHOLD)
    lists = []
    for r in range(64):
        c = np.nonzero(cand[r])[0]
        c = c[np.argsort(t[r, c], kind="stable")]
        T, hits = 1.0, []
        for j in c:  # front to back
            hits.append(near[j])
            T *= 1.0 - alpha[r, j]
            if T < T_THRESHOLD:
                break
        lists.append(hits)
    rows = max(len(h) for h in lists)
    pos = -np.ones((rows, 64), np.int64)
    for r, h in enumerate(lists):
        pos[:len(h), r] = h
    return pos


def presum(pos):
    """The lanes of a row that still own a contribution after the lane ^ 1 and the lane ^ 8 level (the lower lane of an equal pair keeps it)."""
    lane = np.arange(64)
    mine = pos >= 0
    for dlt in (1, 8):
        p = lane ^ dlt
        same = mine & mine[p] & (pos == pos[p])
        mine = mine & ~(same & ((lane & dlt) != 0))
    return mine


def largest_group(pos, mask):
    return int(np.unique(pos[mask], return_counts=True)[1].max()) if mask.any() else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gaussians", type=int, default=1_000_000)
    ap.add_argument("--variant", default="init", choices=["init", "trained"])
    ap.add_argument("--tiles", type=int, default=60)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    a = ap.parse_args()
    g = {k: v.astype(np.float64) for k, v in syn.make_scene(a.gaussians, a.variant, seed=0).items()}
    cam = syn.default_camera()
    opacity = 1.0 / (1.0 + np.exp(-g["opacity"][:, 0]))
    k = 2.0 * EXP_POWER
    sf = np.where(opacity > ALPHA_THRESHOLD, (k * np.log(np.maximum(opacity, 1e-30) / ALPHA_THRESHOLD)) ** (1.0 / k), 0.0)
    s = np.exp(g["scale"]) * sf[:, None]
    q = g["rotation"] / np.linalg.norm(g["rotation"], axis=1, keepdims=True)
    r, x, y, z = q.T
    R = np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y)], -1),
                  np.stack([2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x)], -1),
                  np.stack([2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], -1)], 1)
    Wm = np.swapaxes(R, 1, 2) / s[:, :, None]  # rows of W: R^T scaled by 1 / semi-axis
    pre = (g["mean"], Wm, opacity, sf, s.max(1))
    rng = np.random.default_rng(a.seed)
    tiles = [(int(rng.integers(a.width // 8)), int(rng.integers(a.height // 8))) for _ in range(a.tiles)]
    rows_per_tile, hits, active, distinct, left, rounds, rounds3, steps_dpp, steps_alone, leaders = [], 0, [], [], [], [], [], [], [], []
    for tx, ty in tiles:
        pos = tile_rows(g, cam, a.width, a.height, tx, ty, pre)
        rows_per_tile.append(pos.shape[0])
        hits += int((pos >= 0).sum())
        for row in pos:
            act = row >= 0
            mine = presum(row)
            lane = np.arange(64)
            p2 = lane ^ 2  # a lane ^ 2 level on top (measured and dropped in round 13)
            same = mine & mine[p2] & (row == row[p2])
            mine3 = mine & ~(same & ((lane & 2) != 0))
            active.append(int(act.sum())), distinct.append(len(np.unique(row[act]))), left.append(int(mine.sum()))
            rounds.append(largest_group(row, mine)), rounds3.append(largest_group(row, mine3))
            steps_dpp.append(math.ceil(math.log2(max(largest_group(row, mine), 1)))), steps_alone.append(math.ceil(math.log2(max(largest_group(row, act), 1))))
            leaders.append(len(np.unique(row[mine])))
    rd = np.array(rounds)
    print(f"{a.tiles} tiles of {a.width}x{a.height}, {a.gaussians} gaussians, variant {a.variant}, seed {a.seed}")
    print(f"rows per tile {np.mean(rows_per_tile):.1f}, hits per ray {hits / (64.0 * a.tiles):.2f}")
    print(f"per row: active lanes {np.mean(active):.1f}, distinct gaussians {np.mean(distinct):.1f} (= match iterations = leaders: {np.mean(leaders):.1f}), lanes left after the two DPP levels {np.mean(left):.1f}")
    print(f"table rounds per row (claim-word update, largest group after the DPP levels) {rd.mean():.2f}; 10 % / 90 % quantiles {np.quantile(rd, 0.1):.0f} / {np.quantile(rd, 0.9):.0f}, max {rd.max()}; with a lane ^ 2 level on top {np.mean(rounds3):.2f}")
    print(f"pointer-jumping (tree) steps per row {np.mean(steps_alone):.2f}; behind the two DPP levels {np.mean(steps_dpp):.2f}")


if __name__ == "__main__":
    main()
