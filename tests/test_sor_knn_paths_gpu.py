"""GPU parity of the SOR kNN kernel's paths (csrc/crop.hip sor_knn_kernel): interior queries
(5x5 window + box), border queries (the 9x9 and 17x17 rings added to the kept list),
the brute force (no window reaches 20 points, box rejected, no K, no index map), image-edge
clamping, tiny and empty crops, exact ties. Every case is bit-exact against the oracle, and a
numpy census of the eroded mask first asserts that the classes the case is meant to exercise
are present, so a case cannot pass by missing its path."""
import numpy as np
import pytest
import torch

from oracle import dpfm_oracle as O

pytestmark = pytest.mark.gpu

KNN = 20
FX = 100.0


def _pre_mask(E):
    """A mask whose plus-shaped 3x3 erosion is exactly E (E dilated by the same element)."""
    E = E.astype(bool)
    m = E.copy()
    m[1:, :] |= E[:-1, :]
    m[:-1, :] |= E[1:, :]
    m[:, 1:] |= E[:, :-1]
    m[:, :-1] |= E[:, 1:]
    assert np.array_equal(O.erode_seg_mask(m), E), "the eroded mask is not the intended one"
    return np.where(m, 255, 0).astype(np.uint8)


def _window_counts(E, R):
    """Points in the (2R+1)^2 window (clipped at the image edge) of every pixel."""
    H, W = E.shape
    c = np.zeros((H + 1, W + 1), dtype=np.int64)
    c[1:, 1:] = np.cumsum(np.cumsum(E.astype(np.int64), 0), 1)
    v, u = np.indices((H, W))
    v0, v1 = np.maximum(v - R, 0), np.minimum(v + R, H - 1) + 1
    u0, u1 = np.maximum(u - R, 0), np.minimum(u + R, W - 1) + 1
    return c[v1, u1] - c[v0, u1] - c[v1, u0] + c[v0, u0]


def _classes(E):
    """Per point (row-major order): 0 interior (5x5 holds kk), 1 the 9x9 window suffices,
    2 the 17x17 window is needed, 3 no window reaches kk (brute force)."""
    n = int(E.sum())
    kk = min(KNN, n)
    c5, c9, c17 = (_window_counts(E, R)[E] for R in (2, 4, 8))
    return np.where(c5 >= kk, 0, np.where(c9 >= kk, 1, np.where(c17 >= kk, 2, 3)))


def _tilted(H, W):
    v, u = np.indices((H, W))
    return (800 + 2 * u + 3 * v).astype(np.int16)


def _blob(n, H, W, v0=3, u0=3, width=5):
    E = np.zeros((H, W), dtype=bool)
    for k in range(n):
        E[v0 + k // width, u0 + k % width] = True
    return E


def _comb(n, H, W):
    """Stripes 2 pixels wide, 8 pixels apart, n points: every 5x5 window holds <= 10 points."""
    E = np.zeros((H, W), dtype=bool)
    rows, left, s = 32, n, 0
    while left > 0:
        for r in range(rows):
            for c in range(2):
                if left > 0:
                    E[3 + r, 3 + 8 * s + c] = True
                    left -= 1
        s += 1
    return E


def _scenario(name):
    """-> (eroded masks [F, H, W] bool, depth [F, H, W] int16, K 3x3, expected classes per frame)."""
    K = np.array([[FX, 0.0, 47.5], [0.0, FX, 31.5], [0.0, 0.0, 1.0]])
    if name == "mixed":
        H, W = 64, 96
        E = np.zeros((H, W), dtype=bool)
        E[3:61, 3:23] = True    # blob: interior, edge and corner queries
        E[3:61, 35:38] = True   # 3 px bar: the 9x9 window suffices
        E[3:61, 51:53] = True   # 2 px bar: needs 17x17
        E[3:61, 67] = True      # 1 px line: no window reaches 20
        return E[None], _tilted(H, W)[None], K, [{0, 1, 2, 3}]
    if name == "comb":
        H, W = 64, 96
        Es = np.stack([_comb(n, H, W) for n in (255, 256, 257)])
        return Es, np.stack([_tilted(H, W)] * 3), K, [{2}, {2}, {2}]
    if name == "edges":
        H, W = 24, 40
        E = np.ones((1, H, W), dtype=bool)  # touches row 0, column 0, the last row and column
        return E, _tilted(H, W)[None], K, [{0, 1}]
    if name == "small":
        H, W = 24, 40
        ns = (1, 0, 19, 20, 0, 21)
        Es = np.stack([_blob(n, H, W) for n in ns])
        # kk = min(20, n): a 5-wide blob of 19 / 20 / 21 points has queries whose 5x5 window holds all kk
        # and queries that need the 9x9 ring; the 1-point crop is its own only neighbour
        return Es, np.stack([_tilted(H, W)] * len(ns)), K, [{0}, None, {0, 1}, {0, 1}, None, {0, 1}]
    if name == "ties":
        H, W = 24, 40
        E = np.zeros((1, H, W), dtype=bool)
        E[0, 4:18, 5:25] = True
        return E, np.full((1, H, W), 1000, dtype=np.int16), K, [{0, 1}]
    if name == "boxreject":
        H, W = 24, 40
        E = np.zeros((1, H, W), dtype=bool)
        E[0, 3:19, 4:24] = True
        v, u = np.indices((H, W))
        d = np.where((u + v) % 2 == 0, 500, 5000).astype(np.int16)  # a depth step at every pixel
        return E, d[None], K, [{0}]
    raise KeyError(name)


SCENARIOS = ["mixed", "comb", "edges", "small", "ties", "boxreject"]
_REF = {}  # scenario -> (xyz, off, [avg per frame], [kept per frame]) computed once


def _box_rejections(E, xyz, K):
    """Interior queries of one frame whose camera box is rejected: (Z <= r, Z > r with a box of
    64 px or more). T = the kk-th smallest squared distance in the 5x5 window, as in the kernel."""
    H, W = E.shape
    idx = -np.ones((H, W), dtype=np.int64)
    idx[E] = np.arange(int(E.sum()))
    kk = min(KNN, int(E.sum()))
    near = far = 0
    for v, u in zip(*np.nonzero(E)):
        w = idx[max(v - 2, 0):v + 3, max(u - 2, 0):u + 3]
        w = w[w >= 0]
        if w.size < kk:
            continue
        q = xyz[idx[v, u]]
        d = xyz[w] - q
        T = np.sort((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])[kk - 1]
        r = np.sqrt(T)
        if q[2] <= r:
            near += 1
        elif K[0, 0] * r / q[2] >= 64.0:
            far += 1
    return near, far


@pytest.mark.parametrize("mode", ["K", "noK", "nopix"])
@pytest.mark.parametrize("name", SCENARIOS)
def test_sor_knn_paths(device, name, mode):
    from dpfm_amd import ops
    Es, depth, K, want = _scenario(name)
    F, H, W = Es.shape
    masks = np.stack([_pre_mask(E) for E in Es])
    counts = [int(E.sum()) for E in Es]
    # census: the classes this case is meant to exercise are there
    for f, E in enumerate(Es):
        if want[f] is not None:
            cls = _classes(E)
            assert want[f] <= set(cls.tolist()), (name, f, np.bincount(cls, minlength=4))
            if name == "mixed":  # one 64-point wave and one 256-point tile hold all four classes
                assert set(cls[:64].tolist()) == {0, 1, 2, 3} and set(cls[:256].tolist()) == {0, 1, 2, 3}
            if name == "comb":  # every query of every tile is a border query
                assert (cls != 0).all()
    if name == "comb":
        assert counts == [255, 256, 257]  # a last wave with 63, 64 and 1 active lanes
    if name == "small":
        assert counts == [1, 0, 19, 20, 0, 21]
    if name == "edges":
        E = Es[0]
        assert E[0].any() and E[-1].any() and E[:, 0].any() and E[:, -1].any()

    Kt = torch.from_numpy(np.stack([K.reshape(9)] * F)).to(device)
    cs = torch.ones(F, dtype=torch.float32, device=device)
    bp = ops.backproject(torch.from_numpy(depth).to(device), torch.from_numpy(masks).to(device), Kt, cs,
                         cap=int(sum(counts)) + 1)
    off = bp["off"].cpu().numpy()
    assert (off[1:] - off[:-1]).tolist() == counts
    xyz = bp["xyz"].cpu().numpy()[:off[-1]]
    if name not in _REF:
        crops = [xyz[off[f]:off[f + 1]] for f in range(F)]
        _REF[name] = (xyz.copy(), [O.sor_avg_distances(c) if c.shape[0] else np.zeros(0) for c in crops],
                      [O.remove_outliers_indices(c) for c in crops])
    ref_xyz, ref_avg, ref_keep = _REF[name]
    np.testing.assert_array_equal(xyz, ref_xyz)
    if name == "boxreject" and mode == "K":
        near, far = _box_rejections(Es[0], xyz, K)
        assert near > 0 and far > 0, (near, far)  # Z <= r, and a box of 64 px or more

    kw = dict(want_idx=True)
    if mode != "nopix":
        kw.update(pix=bp["pix"], idxmap=bp["idxmap"])
    if mode == "K":
        kw.update(K=Kt)
    nmax = max(counts)
    res = ops.sor(bp["xyz"], bp["off"], nmax, **kw)
    res2 = ops.sor(bp["xyz"], bp["off"], nmax, **kw)
    avg = res["avg"][:off[-1]]
    assert torch.equal(avg.view(torch.int64), res2["avg"][:off[-1]].view(torch.int64)), "two launches differ"
    assert torch.equal(res["off"], res2["off"]), "two launches differ (kept counts)"
    nk = int(res["off"][-1])
    assert torch.equal(res["kept_idx"][:nk], res2["kept_idx"][:nk]), "two launches differ (kept_idx)"
    avg = avg.cpu().numpy()
    oo = res["off"].cpu().numpy()
    kidx = res["kept_idx"].cpu().numpy()
    for f in range(F):
        np.testing.assert_array_equal(avg[off[f]:off[f + 1]], ref_avg[f], err_msg=f"{name} {mode} avg crop {f}")
        np.testing.assert_array_equal(kidx[oo[f]:oo[f + 1]], ref_keep[f], err_msg=f"{name} {mode} kept crop {f}")
