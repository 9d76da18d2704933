"""Prior views on the GPU (csrc/priors.hip; torch.ops.egr.prior_pairs / prior_fit / prior_finish; priors.py): the projection and the pairs bit for bit against
the numpy restatement (priors_restatement.py), the fit against what the reference's ransac_linear_fit gave (tests/golden/prior_vectors.npz) and against the fp64
fit on its own inliers, the finish against the restatement, and prepare_prior_views end to end into a ViewSet."""
import importlib
from types import SimpleNamespace

import numpy as np
import pytest

import priors_restatement as pr
from test_priors_host import GOLD

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
PKG = "editable-gaussian-reflections_amd"
H, W = 24, 40
F = np.float32


@pytest.fixture(scope="module")
def priors():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU; the product has no CPU fallback")
    mod = importlib.import_module(PKG + ".priors")
    importlib.import_module(PKG).load_library()
    return mod


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(a):
    return np.ascontiguousarray(np.asarray(a, F)).view(np.uint32)


def bit(v):
    return int(np.array([v], F).view(np.uint32)[0])


def ulp(v):
    return float(np.spacing(F(abs(float(v)))))


def gold_view(gold, **more):
    return SimpleNamespace(R=gold["view_R"], T=gold["view_T"], FovX=float(gold["view_fovx"]), FovY=float(gold["view_fovy"]), depth_image=gold["view_depth"],
                           normal_image=gold["view_normal"], metalness_image=gold["view_metalness"], **more)


# ---- projection and pairs
def test_projection_and_pairs_bit_for_bit(priors, gold):
    rng = np.random.default_rng(11)
    fovx = 2 * np.arctan(W / (2 * 16.0))  # fx = 16
    fovy = 2 * np.arctan(H / (2 * 16.0))
    q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    infos = [SimpleNamespace(R=q, T=rng.standard_normal(3), FovX=0.9, FovY=0.6), SimpleNamespace(R=np.eye(3), T=np.zeros(3), FovX=float(fovx), FovY=float(fovy)), gold_view(gold)]
    rows = priors.camera_rows(infos, H, W)
    assert rows[1, 12:16].tolist() == [16.0, 16.0, 20.0, 12.0]
    # view 1, z = 2: behind the camera; outside; u = -0.5 exactly (column 0); u = W - 0.5 exactly (40: outside); three points in pixel (12, 20), the nearest in the middle
    seven = np.array([[0.0, 0.0, -2.0], [9.0, 0.0, 2.0], [-20.5 * 2 / 16, 0.0, 2.0], [19.5 * 2 / 16, 0.25, 2.0], [0.01, 0.0, 3.0], [0.0, 0.02, 1.25], [-0.01, -0.01, 2.5]], F)
    points = [np.zeros((0, 3), F), seven, gold["view_points"]]
    depth = rng.uniform(0.5, 3.0, (3, H, W, 1)).astype(F)
    depth[1, 12, 0, 0] = np.nan  # under the point in column 0: dropped
    depth[2].reshape(-1)[np.flatnonzero(gold["view_sparse"].reshape(-1) != 0)[[5, 77]]] = (np.inf, -np.inf)
    offsets = np.cumsum([0] + [len(p) for p in points]).tolist()
    sparse, px, py, count, dropped = torch.ops.egr.prior_pairs(dev(rows), dev(np.concatenate(points)), offsets, dev(depth))
    sparse, px, py, count, dropped = (t.cpu().numpy() for t in (sparse, px, py, count, dropped))
    want = [pr.project(rows[v], points[v], H, W) for v in range(3)]
    assert not np.isfinite(want[0]).any() and np.isfinite(want[2]).sum() == 300
    assert np.flatnonzero(np.isfinite(want[1]).reshape(-1)).tolist() == [12 * W, 12 * W + 20] and want[1][12, 20] == F(1.25) and want[1][12, 0] == 2.0
    for v in range(3):
        assert np.array_equal(bits(sparse[v]), bits(want[v])), v
        x, y, pix, drops = pr.pairs(want[v], depth[v, :, :, 0])
        assert count[v] == len(x) and dropped[v] == drops, (v, count[v], dropped[v])
        assert np.array_equal(bits(px[v, : len(x)]), bits(x)) and np.array_equal(bits(py[v, : len(y)]), bits(y)), v  # the row-major order
        assert (np.diff(pix) > 0).all()
    assert count.tolist() == [0, 1, 298] and dropped.tolist() == [0, 1, 2]
    # three channels: channel 0 is read
    depth3 = np.concatenate([depth, depth + 1, depth + 2], axis=3)
    again = torch.ops.egr.prior_pairs(dev(rows), dev(np.concatenate(points)), offsets, dev(depth3))
    assert np.array_equal(bits(again[1].cpu().numpy()[2, :298]), bits(px[2, :298])) and again[3].cpu().tolist() == [0, 1, 298]
    # the typed wrapper: camera-space points, 0 = empty
    flat = priors.project_points(seven, float(fovx), float(fovy), (H, W)).cpu().numpy()
    assert np.array_equal(flat, np.where(np.isfinite(want[1]), want[1], F(0)))


# ---- the fit
STRIDE = 80 * 96  # the pair lists of a view of 80 x 96: the 5000-pair case takes more than one pass of the workgroup


def tie_case():
    """600 pairs around y = x, sampled at pairs 0 and 1 (w = 1, b = 0 exactly; top_k = 60): 57 residuals below 0.5, five of exactly 0.5 at pairs 10, 300, 301, 550, 599 -
    in all three chunks of the workgroup -, the rest above 1, except three at x = 0 that differ from 0.5 in the last bits (pair 20 just below: an inlier; pairs 400
    and 401 just above: in other bins of the select's last pass). The first three of the five are inliers. Every residual is exact in fp32."""
    rng = np.random.default_rng(3)
    ties, near = [10, 300, 301, 550, 599], [20, 400, 401]
    x = rng.integers(0, 64, 600).astype(F)
    x[:2] = (0.0, 1.0)
    r = (rng.integers(1100, 4000, 600) / 1024.0).astype(F)
    small = rng.choice(np.array([i for i in range(2, 600) if i not in ties + near]), 54, replace=False)
    r[small] = (rng.choice(np.arange(1, 500), 54, replace=False) / 1024.0).astype(F)
    r[:2], r[ties] = 0.0, 0.5
    x[near], r[near] = 0.0, F([0.5 - 2.0 ** -25, 0.5 + 2.0 ** -24, 0.5 + 5 * 2.0 ** -24])
    assert (r < 0.5).sum() == 57 and (r == 0.5).sum() == 5
    y = (x + r * rng.choice(F([1.0, -1.0]), 600)).astype(F)
    assert np.array_equal(np.abs(y - x), r)
    return x, y, np.array([[0, 1]], np.int32), ties


@pytest.fixture(scope="module")
def fits(priors, gold):
    """ONE call for all the lists - the fixture's cases, N = 2 and 3, the tie - as views of one chunk with different counts, and the same call again."""
    rng = np.random.default_rng(5)
    cases = {}
    for name in ["pairs_%d" % n for n in gold["sizes"]] + ["view"]:
        cases[name] = (gold[name + "_x"], gold[name + "_y"], gold[name + "_table"], int(gold[name + "_mask"].sum()))
    for n in (2, 3):
        x = rng.uniform(0.5, 5.0, n).astype(F)
        cases["tiny_%d" % n] = (x, (1.3 * x + 0.2 + rng.normal(0, 0.01, n)).astype(F), priors.sample_table(n, seed=n), 1)
    tx, ty, ttable, _ = tie_case()
    cases["tie"] = (tx, ty, np.repeat(ttable, 100, axis=0), 60)
    names = list(cases)
    V = len(names)
    X, Y = np.zeros((V, STRIDE), F), np.zeros((V, STRIDE), F)
    table = np.zeros((V, 100, 50), np.int32)
    for v, name in enumerate(names):
        x, y, t, _ = cases[name]
        X[v, : len(x)], Y[v, : len(x)], table[v, :, : t.shape[1]] = x, y, t
    counts, sizes, top_ks = [len(cases[n][0]) for n in names], [cases[n][2].shape[1] for n in names], [cases[n][3] for n in names]
    run = lambda: [t.cpu().numpy() for t in torch.ops.egr.prior_fit(dev(X), dev(Y), counts, sizes, top_ks, torch.from_numpy(table), 0, True)]
    first, second = run(), run()
    out = {}
    for v, name in enumerate(names):
        n = counts[v]
        ab, it, err, hyp_error, hyp_model, mask = (t[v] for t in first)
        out[name] = SimpleNamespace(x=cases[name][0], y=cases[name][1], table=cases[name][2], top_k=top_ks[v], a=ab[0], b=ab[1], it=int(it), error=float(err), hyp_error=hyp_error,
                                    hyp_model=hyp_model, mask=mask[:n].astype(bool), tail=mask[n:])
    out["_runs"] = (first, second)
    return out


def check_self_consistent(c):
    """(a, b) within one fp32 ulp of the fp64 fit on the returned mask; best_error within 1e-12 of the restated error of the returned iteration; the mask is that
    iteration's top_k."""
    x, y = c.x[c.mask].astype(np.float64), c.y[c.mask].astype(np.float64)
    A = np.stack([x, np.ones(len(x))], axis=1)
    a64, b64 = np.linalg.lstsq(A, y, rcond=None)[0]  # (minimum norm where the inliers have no spread in x)
    assert abs(float(c.a) - a64) <= ulp(a64) and abs(float(c.b) - b64) <= ulp(b64), (c.a, a64, c.b, b64)
    w, b, thr_bits, take, error = pr.hypothesis(c.x, c.y, np.asarray(c.table[c.it], np.int64), c.top_k)
    assert abs(c.error - error) <= 1e-12 * abs(error), (c.error, error)
    assert c.error == c.hyp_error[c.it]
    assert [bit(m) for m in c.hyp_model[c.it]] == [bit(w), bit(b), int(thr_bits), take]
    assert np.array_equal(c.mask, pr.inliers_of(c.x, c.y, w, b, thr_bits, take)) and c.mask.sum() == c.top_k and not c.tail.any()


@pytest.mark.parametrize("name", ["pairs_21", "pairs_64", "pairs_257", "pairs_1000", "pairs_5000", "view"])
def test_fit_against_the_reference(fits, gold, name):
    c = fits[name]
    a, b = float(gold[name + "_a"]), float(gold[name + "_b"])
    print(name, "a", c.a, a, "b", c.b, b, "iteration", c.it, "error", c.error)
    assert abs(float(c.a) - a) <= float(gold["tol_a"]) * abs(a) and abs(float(c.b) - b) <= float(gold["tol_b"])
    assert np.array_equal(c.mask, gold[name + "_mask"]) and c.it == int(gold[name + "_best_iteration"])
    check_self_consistent(c)
    # every hypothesis, not only the best: errors against the restatement
    restated = pr.ransac(c.x, c.y, c.table, c.top_k)
    np.testing.assert_allclose(c.hyp_error, restated["errors"], rtol=1e-12, atol=0)


def test_fit_histogram_passes_are_spread(fits):
    """What makes these cases tests of the radix select: the residuals that share the threshold's digits so far fall into several bins - in the first three
    passes of the 5000-pair case, and in the last pass of the tie case, whose neighbours of the threshold differ from it in the last byte only."""
    for name, shifts in (("pairs_5000", (24, 16, 8)), ("tie", (24, 16, 0))):
        c = fits[name]
        r = bits(pr.residuals(c.x, c.y, c.hyp_model[c.it, 0], c.hyp_model[c.it, 1])).astype(np.uint64)
        thr = bit(c.hyp_model[c.it, 2])
        for shift in shifts:
            same = r[(r >> (shift + 8)) == (thr >> (shift + 8))]
            assert len(np.unique((same >> shift) & 255)) >= 2, (name, shift)


@pytest.mark.parametrize("n", [2, 3])
def test_fit_of_two_and_three_pairs(fits, n):
    c = fits["tiny_%d" % n]
    check_self_consistent(c)
    restated = pr.ransac(c.x, c.y, c.table, 1)
    assert c.error <= restated["errors"].min() * (1 + 1e-6) + 1e-30
    i = int(np.flatnonzero(c.mask)[0])  # one inlier: no spread, the minimum-norm refit
    scale = float(c.y[i]) / (float(c.x[i]) ** 2 + 1.0)
    assert abs(float(c.a) - scale * float(c.x[i])) <= ulp(scale * float(c.x[i])) and abs(float(c.b) - scale) <= ulp(scale)


def test_fit_threshold_tie_goes_by_pair_order(fits):
    c = fits["tie"]
    ties = tie_case()[3]
    check_self_consistent(c)
    assert c.it == 0 and bit(c.hyp_model[0, 3]) == 3 and c.hyp_model[0, 2] == 0.5  # every iteration is the same hypothesis: the lowest wins
    assert c.mask[ties].tolist() == [True, True, True, False, False]
    assert c.mask[[20, 400, 401]].tolist() == [True, False, False]


def test_fit_twice_gives_the_same_bits(fits):
    first, second = fits["_runs"]
    for a, b in zip(first, second):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))


def test_fit_wrapper_and_least_squares(priors, gold):
    x, y = gold["pairs_1000_x"], gold["pairs_1000_y"]
    (a, b), mask, more = priors.ransac_linear_fit(x, y, seed=int(gold["pairs_1000_seed"]), details=True)
    assert a.is_cuda and a.dim() == 0 and mask.dtype == torch.bool and mask.shape == (1000,)
    assert np.array_equal(mask.cpu().numpy(), gold["pairs_1000_mask"]) and int(more.best_iteration) == int(gold["pairs_1000_best_iteration"]) and more.top_k == 100
    assert abs(float(a) - float(gold["pairs_1000_a"])) <= float(gold["tol_a"]) * float(gold["pairs_1000_a"]) and abs(float(b) - float(gold["pairs_1000_b"])) <= float(gold["tol_b"])
    (a, b), mask = priors.ransac_linear_fit(x, y, method="lstsq")
    A = np.stack([x.astype(np.float64), np.ones(1000)], axis=1)
    a64, b64 = np.linalg.lstsq(A, y.astype(np.float64), rcond=None)[0]
    assert abs(float(a) - a64) <= ulp(a64) and abs(float(b) - b64) <= ulp(b64) and bool(mask.all())
    with pytest.raises(RuntimeError, match="sample index 1000"):  # the table is checked on the host
        torch.ops.egr.prior_fit(dev(x[None]), dev(y[None]), [1000], [2], [100], torch.tensor([[[0, 1000]]], dtype=torch.int32), 0, False)
    with pytest.raises(ValueError, match="at least 2"):
        priors.ransac_linear_fit(x[:1], y[:1])


# ---- the finish
def test_finish_against_the_restatement(priors):
    rng = np.random.default_rng(21)
    V = 2
    infos = []
    for _ in range(V):
        q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
        infos.append(SimpleNamespace(R=q, T=rng.standard_normal(3), FovX=float(rng.uniform(0.6, 1.2)), FovY=float(rng.uniform(0.4, 0.9))))
    rows = priors.camera_rows(infos, H, W)
    depth = rng.uniform(0.2, 4.0, (V, H, W, 3)).astype(F)
    normal = rng.standard_normal((V, H, W, 3)).astype(F)
    normal[1, 3, 4] = 0.0  # a zero normal
    metal = rng.random((V, H, W)).astype(F)
    metal[0, 0, :3] = (0.0, 1.0, 0.5)
    ab = np.array([[2.1, 0.25], [0.7, 0.1]], F)
    distance, world, f0 = (t.cpu().numpy() for t in torch.ops.egr.prior_finish(dev(rows), dev(ab), dev(depth), dev(normal), dev(metal)))
    assert distance.shape == (V, H, W, 1) and world.shape == (V, H, W, 3) and f0.shape == (V, H, W, 3)
    for v in range(V):
        want_d, want_n, want_f0 = pr.finish(rows[v], ab[v, 0], ab[v, 1], depth[v, :, :, 0], normal[v], metal[v])
        assert np.array_equal(bits(f0[v]), bits(want_f0))
        np.testing.assert_allclose(distance[v, :, :, 0], want_d, rtol=4 * 2.0 ** -23, atol=0)
        ok = np.isfinite(want_n).all(axis=-1)
        assert np.abs(world[v][ok] - want_n[ok]).max() <= 8 * 2.0 ** -24
        assert np.array_equal(np.isnan(world[v]), np.isnan(want_n))
    assert np.isnan(world[1, 3, 4]).all() and np.isnan(world).sum() == 3
    # without metalness there is no f0; one channel of depth gives the same distance as channel 0 of three
    d1, n1, none = torch.ops.egr.prior_finish(dev(rows), dev(ab), dev(depth[..., :1]), dev(normal), None)
    assert none.numel() == 0 and np.array_equal(bits(d1.cpu().numpy()), bits(distance)) and np.array_equal(bits(n1.cpu().numpy()), bits(world))


def test_finish_refuses_an_overlapping_output_with_nothing_written(priors):
    cabi = importlib.import_module(PKG + ".c_abi")
    rng = np.random.default_rng(2)
    rows = dev(priors.camera_rows([SimpleNamespace(R=np.eye(3), T=np.zeros(3), FovX=0.9, FovY=0.6)], H, W))
    ab, depth, normal = dev(np.array([[2.0, 1.0]], F)), dev(rng.uniform(1, 2, (1, H, W, 1)).astype(F)), dev(rng.standard_normal((1, H, W, 3)).astype(F))
    distance, world = torch.full((1, H, W, 1), -7.0, device="cuda"), torch.full((1, H, W, 3), -7.0, device="cuda")
    before = depth.clone(), normal.clone()
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream().cuda_stream
    with pytest.raises(RuntimeError, match="egr_prior_finish: an output overlaps an input"):  # in place
        cabi.prior_finish(1, H, W, rows.data_ptr(), ab.data_ptr(), depth.data_ptr(), normal.data_ptr(), depth.data_ptr(), world.data_ptr(), stream=stream)
    with pytest.raises(RuntimeError, match="egr_prior_finish: two outputs overlap"):
        cabi.prior_finish(1, H, W, rows.data_ptr(), ab.data_ptr(), depth.data_ptr(), normal.data_ptr(), world.data_ptr() + 4 * H * W, world.data_ptr(), stream=stream)
    torch.cuda.synchronize()
    assert torch.equal(depth, before[0]) and torch.equal(normal, before[1]) and bool((distance == -7).all()) and bool((world == -7).all())
    cabi.prior_finish(1, H, W, rows.data_ptr(), ab.data_ptr(), depth.data_ptr(), normal.data_ptr(), distance.data_ptr(), world.data_ptr(), stream=stream)  # the same call, out of place
    torch.cuda.synchronize()
    want = torch.ops.egr.prior_finish(rows, ab, depth, normal, None)
    assert torch.equal(distance, want[0]) and torch.equal(world, want[1])


# ---- end to end
def test_prepare_prior_views_end_to_end(priors, gold):
    ds = importlib.import_module(PKG + ".dataset")
    seed = int(gold["view_seed"])
    info = gold_view(gold, image=np.full((H, W, 3), 0.5, F), tag="kept")
    rec = priors.prepare_prior_views([info], [gold["view_points"]], seed=seed)[0]
    fit = rec.depth_fit
    a, b, ref_a, ref_b = float(fit.a), float(fit.b), float(gold["view_a"]), float(gold["view_b"])
    tol_a, tol_b = float(gold["tol_a"]), float(gold["tol_b"])
    print("a", a, ref_a, "b", b, ref_b)
    assert (fit.num_pairs, fit.top_k, fit.dropped, fit.fitted, int(fit.best_iteration)) == (300, 30, 0, True, int(gold["view_best_iteration"]))
    assert abs(a - ref_a) <= tol_a * abs(ref_a) and abs(b - ref_b) <= tol_b
    assert rec.tag == "kept" and rec.image is info.image and rec.metalness_image is info.metalness_image  # passed through untouched
    distance, world, f0 = rec.depth_image.cpu().numpy(), rec.normal_image.cpu().numpy(), rec.f0_image.cpu().numpy()
    assert distance.shape == (H, W, 1) and world.shape == (H, W, 3) and f0.shape == (H, W, 3) and rec.depth_image.is_cuda
    assert np.array_equal(bits(f0), bits(gold["view_f0"]))
    assert np.abs(world - gold["view_normal_world"]).max() <= 8 * 2.0 ** -24
    # the distance: the fit's tolerance through Z = x a + b, times the ray's length per unit depth, plus the roundings of the chain itself
    row = priors.camera_rows([info], H, W)[0].astype(np.float64)
    u, v = np.meshgrid(np.arange(W), np.arange(H))
    per_depth = np.sqrt(((u - row[14]) / row[12]) ** 2 + ((v - row[15]) / row[13]) ** 2 + 1.0)
    x = gold["view_depth"][:, :, 0].astype(np.float64)
    bound = per_depth * (tol_a * np.abs(x * ref_a) + tol_b) + 4 * 2.0 ** -23 * np.abs(gold["view_distance"][:, :, 0])
    assert (np.abs(distance[:, :, 0].astype(np.float64) - gold["view_distance"][:, :, 0]) <= bound).all()
    # into a ViewSet as they are: the depth plane is half(distance), znear / zfar follow
    vs = ds.ViewSet(H, W, 1)
    vs.add([rec])
    half = rec.depth_image.half()
    assert torch.equal(vs.planes[ds.DEPTH][0, 0], half[:, :, 0]) and torch.equal(vs.planes[4][0], rec.normal_image.half().permute(2, 0, 1)) and vs.present[6]
    assert float(vs.znear[0]) == float(half.float().min() * 0.8) and float(vs.zfar[0]) == float(half.float().max() * 1.5)


def test_prepare_prior_views_in_chunks_with_different_point_counts(priors, gold):
    pts = gold["view_points"]
    lists = [pts, pts[:150], pts[:1], pts[:40], np.zeros((0, 3), F)]
    infos = [gold_view(gold, uid=i) for i in range(5)]
    with pytest.raises(ValueError, match="view 2 has 1 "):
        priors.prepare_prior_views(infos, lists, views_per_call=2, seed=9)
    recs = priors.prepare_prior_views(infos, lists, views_per_call=2, seed=9, on_too_few="identity")  # chunks of 2, 2 and 1 views
    assert [r.depth_fit.num_pairs for r in recs] == [300, 150, 1, 40, 0] and [r.depth_fit.fitted for r in recs] == [True, True, False, True, False]
    assert [r.uid for r in recs] == list(range(5))
    for i, r in enumerate(recs):
        alone = priors.prepare_prior_views([infos[i]], [lists[i]], seed=9 + i, on_too_few="identity")[0]  # view i draws from random.Random(seed + i)
        for got, want in ((r.depth_fit.a, alone.depth_fit.a), (r.depth_fit.b, alone.depth_fit.b), (r.depth_image, alone.depth_image), (r.normal_image, alone.normal_image)):
            assert torch.equal(got, want), i
        assert int(r.depth_fit.best_iteration) == int(alone.depth_fit.best_iteration)
    for i in (2, 4):  # not fitted: the identity
        assert (float(recs[i].depth_fit.a), float(recs[i].depth_fit.b), int(recs[i].depth_fit.best_iteration)) == (1.0, 0.0, -1)
    lsq = priors.prepare_prior_views(infos[:2], lists[:2], method="lstsq")
    x, y, _, _ = pr.pairs(pr.project(priors.camera_rows(infos[:1], H, W)[0], pts[:150], H, W), gold["view_depth"][:, :, 0])
    a64, b64 = np.linalg.lstsq(np.stack([x.astype(np.float64), np.ones(len(x))], axis=1), y.astype(np.float64), rcond=None)[0]
    assert abs(float(lsq[1].depth_fit.a) - a64) <= ulp(a64) and abs(float(lsq[1].depth_fit.b) - b64) <= ulp(b64) and int(lsq[1].depth_fit.best_iteration) == -1
