"""distCUDA2 replacement (csrc/knn.hip) against the brute-force / kd-tree restatement in oracle/knn.py."""
import importlib
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import knn as oknn  # noqa: E402

torch = pytest.importorskip("torch")
PKG = "editable-gaussian-reflections_amd"


def test_restatements_agree():
    rng = np.random.default_rng(0)
    p = rng.normal(size=(700, 3)).astype(np.float32)
    p[10] = p[11]  # a duplicate pair: distance 0 counts
    a, b = oknn.dist2_bruteforce(p), oknn.dist2_kdtree(p)
    np.testing.assert_allclose(a, b, rtol=1e-10, atol=1e-14)
    # hand-checked: 4 points on a line at 0, 1, 3, 7 -> for x=0 the neighbours are at 1, 3, 7: (1 + 9 + 49) / 3
    q = np.array([[0, 0, 0], [1, 0, 0], [3, 0, 0], [7, 0, 0]], np.float32)
    np.testing.assert_allclose(oknn.dist2_bruteforce(q), [59 / 3, (1 + 4 + 36) / 3, (4 + 9 + 16) / 3, (16 + 36 + 49) / 3])


@pytest.fixture(scope="module")
def knn():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU; the product has no CPU fallback")
    return importlib.import_module(PKG + ".simple_knn")


@pytest.mark.gpu
@pytest.mark.parametrize("n", [4, 5, 63, 1025, 5000])
def test_matches_brute_force(knn, n):
    rng = np.random.default_rng(n)
    p = (rng.normal(size=(n, 3)) * np.array([1.0, 3.0, 0.2])).astype(np.float32)
    if n > 100:
        p[7] = p[50]  # duplicates
        p[n // 2:n // 2 + 40, 2] = 0.0  # a coplanar cluster
    out = knn.distCUDA2(torch.from_numpy(p).cuda()).cpu().numpy()
    ref = oknn.dist2_bruteforce(p)
    np.testing.assert_allclose(out, ref, rtol=2e-5, atol=1e-9)


@pytest.mark.gpu
def test_tiny_and_degenerate_inputs(knn):
    assert knn.distCUDA2(torch.zeros(0, 3).cuda()).shape == (0,)
    assert float(knn.distCUDA2(torch.zeros(1, 3).cuda())[0]) == 0.0
    two = knn.distCUDA2(torch.tensor([[0.0, 0, 0], [2.0, 0, 0]]).cuda()).cpu().numpy()
    np.testing.assert_allclose(two, [4.0, 4.0])
    same = knn.distCUDA2(torch.ones(100, 3).cuda()).cpu().numpy()  # all coincident
    assert np.all(same == 0.0)
    with pytest.raises(RuntimeError):
        knn.distCUDA2(torch.zeros(8, 3))  # CPU tensor: no CPU path
    with pytest.raises(RuntimeError):
        knn.distCUDA2(torch.zeros(8, 2).cuda())


@pytest.mark.gpu
def test_scene_scale_init_1m_points(knn):
    """The reference's use (gaussian_model.py:197-201) at full size: 1M surface points, checked against the kd-tree."""
    syn = importlib.import_module(PKG + ".synthetic")
    g = syn.make_scene(1_000_000, "init", seed=3)
    p = g["mean"].astype(np.float32)
    t = torch.from_numpy(p).cuda()
    out = knn.distCUDA2(t)
    torch.cuda.synchronize()
    import time
    t0 = time.perf_counter()
    out = knn.distCUDA2(t)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    sub = np.random.default_rng(0).choice(len(p), 20000, replace=False)
    from scipy.spatial import cKDTree
    d, _ = cKDTree(p.astype(np.float64)).query(p[sub].astype(np.float64), k=4)
    ref = (d[:, 1:] ** 2).mean(1)
    np.testing.assert_allclose(out.cpu().numpy()[sub], ref, rtol=5e-5, atol=1e-10)
    scales = torch.log(torch.sqrt(torch.clamp_min(out, 1e-7)))  # what the caller derives
    assert bool(torch.isfinite(scales).all())
    print(f"distCUDA2 1M points: {dt * 1e3:.1f} ms")
    assert dt < 2.0


# ---- distCUDA2 against the fp64 brute force at the shapes and values where the box search can go wrong ----
# Bar: rtol 1e-6, atol 0. Three subtractions (each counted twice: it is squared), three squares, two adds, the 3-sum and the division are at most 8 roundings,
# 8 * 2^-24 = 4.8e-7; an exact zero has to come out as exactly 0. The reference is O(N^2) in fp64, so n stays at or below 3100.
from hip_common import report  # noqa: E402

RTOL = 1e-6


def run_knn(knn, p):
    return knn.distCUDA2(torch.from_numpy(np.ascontiguousarray(p, np.float32)).cuda()).cpu().numpy()


def against_brute_force(knn, p, name):
    p = np.ascontiguousarray(p, np.float32)
    out, ref = run_knn(knn, p), oknn.dist2_bruteforce(p)
    assert out.dtype == np.float32 and out.shape == (len(p),)
    nz = ref > 0
    worst = float((np.abs(out[nz] - ref[nz]) / ref[nz]).max()) if nz.any() else 0.0
    report("knn_" + name, n=len(p), max_rel_err=f"{worst:.2e}", bar=RTOL)
    np.testing.assert_allclose(out, ref, rtol=RTOL, atol=0)
    return out, ref


@pytest.mark.gpu
@pytest.mark.parametrize("n", [2, 3, 4, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049, 3000])
def test_box_and_wave_boundaries(knn, n):
    """Fewer than four points, one wave and one more, the 1024-point box exactly, one less and one more, two boxes, an odd size: uniform in a box around 0."""
    p = np.random.default_rng(n).uniform([-3.0, -1.0, -20.0], [2.0, 4.0, 5.0], size=(n, 3))
    against_brute_force(knn, p, f"uniform_n{n}")


@pytest.mark.gpu
def test_lattice_ties_are_exact(knn):
    """12^3 integer lattice, shuffled: every point has at least three neighbours at distance exactly 1 and many more tied behind them (box distances tie with the
    running third-best too: the prune is `<=`). Bit-equal 1.0; scaled by 1/4 and shifted, all of it exact in fp32, bit-equal 1/16."""
    ax = np.arange(12, dtype=np.float64)
    p = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3)
    p = p[np.random.default_rng(12).permutation(len(p))]
    out, _ = against_brute_force(knn, p, "lattice")
    assert np.array_equal(out, np.ones(len(p), np.float32))
    q = p * 0.25 + np.array([-100.0, 7.0, 1000.0])
    assert np.array_equal(q.astype(np.float32).astype(np.float64), q)
    out, _ = against_brute_force(knn, q, "lattice_scaled_shifted")
    assert np.array_equal(out, np.full(len(p), 0.0625, np.float32))


@pytest.mark.gpu
def test_cloud_collapsed_into_one_morton_cell(knn):
    """2500 points in a cube of side 1e-5 and one at (1e6, 1e6, 1e6): the frame is 1e6 wide, a Morton cell 0.48, so all keys but one are equal and the sort orders
    nothing; the three boxes overlap completely."""
    rng = np.random.default_rng(21)
    p = np.concatenate([rng.uniform(-0.5e-5, 0.5e-5, size=(2500, 3)), [[1e6, 1e6, 1e6]]])
    p = p[rng.permutation(len(p))]
    against_brute_force(knn, p, "collapsed")


@pytest.mark.gpu
def test_degenerate_frame_axes_and_negative_coordinates(knn):
    rng = np.random.default_rng(22)
    line = np.zeros((2000, 3))
    line[:, 0] = rng.uniform(-7.0, 9.0, 2000)  # hi > lo is false on y and z
    against_brute_force(knn, line, "x_axis")
    plane = rng.uniform(-2.0, 2.0, size=(2000, 3))
    plane[:, 2] = -3.0
    against_brute_force(knn, plane, "plane_z")
    against_brute_force(knn, rng.uniform(-5.0, -4.0, size=(1500, 3)), "negative_only")


@pytest.mark.gpu
def test_coincident_points_count_as_neighbours(knn):
    rng = np.random.default_rng(23)
    p = rng.uniform(-1.0, 1.0, size=(1500, 3)).astype(np.float32)
    same = [3, 400, 401, 1024, 1499]
    p[same] = p[same[0]]
    out, ref = against_brute_force(knn, p, "five_coincident")
    assert np.all(out[same] == 0.0) and np.all(ref[same] == 0.0)
    d = np.linalg.norm(p.astype(np.float64) - p[same[0]].astype(np.float64), axis=1)
    near = np.argsort(d)[5:8]  # the nearest other points: their three nearest include the five
    assert np.all(out[near] > 0.0)


@pytest.mark.gpu
def test_non_finite_rows_are_ignored_and_return_zero(knn):
    """What the `v == v` guards and the ordered compares of csrc/knn.hip give: a row with a NaN or an infinite coordinate is nobody's neighbour and has none."""
    p = np.random.default_rng(24).uniform(-2.0, 3.0, size=(1500, 3)).astype(np.float32)
    p[10, 1] = np.nan
    p[500] = np.nan
    p[1499, 0] = np.inf
    bad = np.array([10, 500, 1499])
    finite = np.setdiff1d(np.arange(1500), bad)
    out = run_knn(knn, p)
    ref = oknn.dist2_bruteforce(p[finite])
    worst = float((np.abs(out[finite] - ref) / ref).max())
    report("knn_non_finite_rows", max_rel_err=f"{worst:.2e}", out_bad=out[bad].tolist())
    np.testing.assert_allclose(out[finite], ref, rtol=RTOL, atol=0)
    assert np.array_equal(out[bad], np.zeros(3, np.float32))


@pytest.mark.gpu
def test_input_forms_give_the_contiguous_fp32_result(knn):
    p = np.random.default_rng(25).uniform(-4.0, 4.0, size=(1100, 3)).astype(np.float32)
    t = torch.from_numpy(p).cuda()
    base = knn.distCUDA2(t)
    np.testing.assert_allclose(base.cpu().numpy(), oknn.dist2_bruteforce(p), rtol=RTOL, atol=0)
    view = t.t().contiguous().t()  # [3,N].T
    assert not view.is_contiguous() and torch.equal(knn.distCUDA2(view), base)
    out64 = knn.distCUDA2(t.double())
    assert out64.dtype == torch.float32 and torch.equal(out64, base)
    h = t.half()
    out16 = knn.distCUDA2(h)
    assert torch.equal(out16.float(), knn.distCUDA2(h.float()))
    np.testing.assert_allclose(out16.float().cpu().numpy(), oknn.dist2_bruteforce(h.float().cpu().numpy()), rtol=RTOL, atol=0)
