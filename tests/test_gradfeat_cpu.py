"""CPU: construction and state-dict names of the networks with gradient features, the
GradOperator container (COO round trip, inverted index), collate(grads=True), and properties of the
operator's restatement (tests/_gradfeat_ref.py) that the GPU tests compare the kernels against."""
import numpy as np
import pytest
import torch

import _gradfeat_ref as R


def test_diffusion_net_with_gradient_features_constructs():
    from dpfm_amd.diffusion_net import DiffusionNet
    net = DiffusionNet(3, 32, C_width=64, N_block=2, with_gradient_features=True)
    sd = net.state_dict()
    for i in range(2):
        assert tuple(sd[f"block_{i}.gradient_features.A_re.weight"].shape) == (64, 64)
        assert tuple(sd[f"block_{i}.gradient_features.A_im.weight"].shape) == (64, 64)
        assert tuple(sd[f"block_{i}.mlp.miniMLP_mlp_layer_000.weight"].shape) == (64, 192)
        assert tuple(sd[f"block_{i}.mlp.miniMLP_mlp_layer_000.bias"].shape) == (64,)
        assert tuple(sd[f"block_{i}.mlp.miniMLP_mlp_layer_001.weight"].shape) == (64, 64)
        assert tuple(sd[f"block_{i}.mlp.miniMLP_mlp_layer_002.weight"].shape) == (64, 64)
        assert tuple(sd[f"block_{i}.diffusion.diffusion_time"].shape) == (64,)
    assert not any(k.endswith("A_re.bias") or k.endswith("A_im.bias") for k in sd)
    # the restatement's names and shapes are the module's (it loads the module's weights strictly)
    ref = R.DiffusionNet(3, 32, 64, 2)
    assert {k: tuple(v.shape) for k, v in ref.state_dict().items()} == {k: tuple(v.shape) for k, v in sd.items()}
    # the upstream default signature constructs (with_gradient_features=True is its default)
    DiffusionNet(3, 32)


def test_without_rotations_has_single_weight():
    from dpfm_amd.diffusion_net import DiffusionNet
    sd = DiffusionNet(3, 32, C_width=64, N_block=1, with_gradient_features=True,
                      with_gradient_rotations=False).state_dict()
    assert tuple(sd["block_0.gradient_features.A.weight"].shape) == (64, 64)
    assert not any("A_re" in k or "A_im" in k for k in sd)


def test_default_dpfmnet_keys_unchanged():
    from dpfm_amd.models.dpfm import DPFMNet
    a, b = DPFMNet().state_dict(), DPFMNet(with_gradient_features=False).state_dict()
    assert list(a) == list(b)
    assert not any("gradient_features" in k for k in a)
    assert tuple(a["feature_extractor.block_0.mlp.miniMLP_mlp_layer_000.weight"].shape) == (64, 128)
    g = DPFMNet(with_gradient_features=True).state_dict()
    assert set(a) < set(g)
    assert tuple(g["feature_extractor.block_1.gradient_features.A_im.weight"].shape) == (64, 64)
    assert tuple(g["feature_extractor.block_0.mlp.miniMLP_mlp_layer_000.weight"].shape) == (64, 192)


def _ragged_operator():
    """Two crops (7 and 4 points) with rows of unequal length, one isolated point."""
    from dpfm_amd.geometry import GradOperator
    rng = np.random.default_rng(3)
    nbr0 = np.full((7, 4), -1, np.int32)
    for i, row in enumerate([[3, 1], [0, 2, 5, 6], [1], [], [6, 0, 2], [1, 4, 3, 0], [5]]):
        nbr0[i, :len(row)] = row
    nbr1 = np.array([[1, 2, 3], [0, -1, -1], [3, 0, -1], [2, -1, -1]], np.int32)
    idx = np.full((2, 7, 5), -1, np.int32)
    val = np.zeros((2, 7, 5, 2))
    for b, nbr in enumerate((nbr0, nbr1)):
        n = nbr.shape[0]
        idx[b, :n, 0] = np.arange(n)
        idx[b, :n, 1:1 + nbr.shape[1]] = nbr
        val[b] = np.where((idx[b] >= 0)[..., None], rng.normal(size=(7, 5, 2)), 0.0)
    return GradOperator.build(torch.from_numpy(idx), torch.from_numpy(val), [7, 4])


def test_grad_operator_coo_round_trip():
    from dpfm_amd.geometry import GradOperator
    op = _ragged_operator()
    coos = [op.coo(b) for b in range(2)]
    assert tuple(coos[0][0].shape) == (7, 7) and tuple(coos[1][1].shape) == (4, 4)
    back = GradOperator.from_coo([c[0] for c in coos], [c[1] for c in coos])
    assert back.idx.shape == (2, 7, 5) and back.counts == (7, 4)  # W = the longest row (4 + the diagonal)
    for b in range(2):
        for got, exp in zip(back.coo(b), coos[b]):
            assert torch.equal(got.indices(), exp.indices())
            assert torch.equal(got.values(), exp.values())
        # dense values equal the slots' (no entry lost or merged)
        gx, gy = R.dense(op.idx[b].numpy(), op.val[b].numpy(), op.counts[b])
        assert np.array_equal(coos[b][0].to_dense().numpy(), gx)
        assert np.array_equal(coos[b][1].to_dense().numpy(), gy)
    assert (back.idx[1, 4:] == -1).all() and (back.val[1, 4:] == 0).all()


def test_grad_operator_inverted_index():
    op = _ragged_operator()
    B, N, W = op.idx.shape
    for b in range(B):
        idx = op.idx[b].reshape(-1).numpy()
        ptr, src = op.tptr[b].numpy(), op.tsrc[b].numpy()
        assert ptr[0] == 0 and ptr[-1] == int((idx >= 0).sum())
        seen = []
        for j in range(N):
            lst = src[ptr[j]:ptr[j + 1]]
            assert (idx[lst] == j).all()
            assert (np.diff(lst) > 0).all()  # ascending (row, slot)
            seen += lst.tolist()
        assert sorted(seen) == np.nonzero(idx >= 0)[0].tolist()  # every non-empty slot exactly once


def test_collate_grads():
    from dpfm_amd.dataset.helpers import collate
    from dpfm_amd.geometry import GradOperator
    op = _ragged_operator()
    rng = np.random.default_rng(0)
    items = []
    for b, n in enumerate((7, 4)):
        gx, gy = op.coo(b)
        shape = {"xyz": rng.normal(size=(n, 3)), "mass": rng.uniform(size=n), "evals": rng.uniform(size=8),
                 "evecs": rng.normal(size=(n, 8)), "L": gx, "gradX": gx, "gradY": gy}
        items.append((dict(shape), dict(shape), {"obj_id": 1}))
    cad, pc, _ = collate(items)
    assert cad["gradX"] is None and cad["gradY"] is None and "grad" not in cad
    cad, pc, _ = collate(items, grads=True)
    assert cad["gradX"] is None and cad["gradY"] is None
    for part in (cad, pc):
        g = part["grad"]
        assert isinstance(g, GradOperator) and g.val.dtype == torch.float32 and g.idx.shape[:2] == (2, 7)
        for b in range(2):
            for got, exp in zip(g.coo(b), op.coo(b)):
                assert torch.equal(got.indices(), exp.indices())
                assert torch.equal(got.values(), exp.values().float())


def test_reference_rows_sum_to_zero():
    pts = R.sphere_cap(70, 0)
    frames = R.tangent_frames(pts)
    for rev in (False, True):
        _, val = R.grad_rows(pts, frames, R.cloud_neighbors(pts, 30), rev=rev)
        big = np.abs(val).max(axis=(1, 2))
        assert (np.abs(val.sum(axis=1)).max(axis=1) <= 1e-12 * big).all()


def test_reference_recovers_linear_gradient_on_plane():
    rng = np.random.default_rng(0)
    pts = np.concatenate((rng.uniform(size=(200, 2)), np.zeros((200, 1))), axis=1)
    normals = np.tile(np.array([0.0, 0.0, 1.0]), (200, 1))
    frames = R.tangent_frames(normals)
    idx, val = R.grad_rows(pts, frames, R.cloud_neighbors(pts, 30))
    gx, gy = R.dense(idx, val, 200)
    a = np.array([0.7, -1.3, 0.4])
    f = pts @ a
    exp_x, exp_y = frames[:, 0] @ a, frames[:, 1] @ a  # the gradient's tangent components
    err = max(np.abs(gx @ f - exp_x).max(), np.abs(gy @ f - exp_y).max())
    print("plane gradient relative error", err / np.linalg.norm(a[:2]))
    assert err <= 1e-4 * np.linalg.norm(a[:2])


def test_hub_precondition():
    """The hub cloud of the transposed-apply test: the centre's in-degree is 60 (twice k), every
    other point's at most 31."""
    pts = R.hub_ring()
    nbr = R.cloud_neighbors(pts, 30)
    indeg = np.bincount(nbr[nbr >= 0], minlength=61)
    assert indeg[60] == 60 and indeg[:60].max() <= 31, (indeg[60], indeg[:60].max())


def test_missing_grad_raises_value_error():
    from dpfm_amd.models.dpfm import DPFMNet
    net = DPFMNet(with_gradient_features=True)
    z = lambda *s: torch.zeros(*s)  # noqa: E731
    shape = {"xyz": z(1, 8, 3), "mass": z(1, 8), "evals": z(1, 64), "evecs": z(1, 8, 64)}
    with pytest.raises(ValueError, match=r'batch\["shape1"\]\["grad"\]'):
        net({"shape1": dict(shape), "shape2": dict(shape)})
