"""GPU: the gradient operators (pk_grad_build, geometry.GradOperator) against the fp64 restatement
in tests/_gradfeat_ref.py, on clouds (30 nearest neighbours) and meshes (edge neighbours), and end
to end through get_operators and the operator cache format."""
import numpy as np
import pytest
import torch

import _gradfeat_ref as R

pytestmark = pytest.mark.gpu


def _check_rows(idx_dev, val_dev, clouds, frames, tables):
    """idx exact; val within 100 x the largest difference between the restatement's two summation
    orders, both relative to each row's largest entry."""
    fwd = [R.grad_rows(p, f, t) for p, f, t in zip(clouds, frames, tables)]
    rev = [R.grad_rows(p, f, t, rev=True) for p, f, t in zip(clouds, frames, tables)]
    nmax = idx_dev.shape[1]
    idx_ref, val_ref = R.fixed_width(fwd, nmax)
    _, val_rev = R.fixed_width(rev, nmax)
    assert np.array_equal(idx_dev, idx_ref)
    big = np.maximum(np.abs(val_ref).max(axis=(2, 3)), 1e-300)  # [B, nmax]
    order = (np.abs(val_ref - val_rev).max(axis=(2, 3)) / big).max()
    err = (np.abs(val_dev - val_ref).max(axis=(2, 3)) / big).max()
    print(f"summation-order difference {order:.3e}, device error {err:.3e}")
    assert order > 0
    assert err <= 100 * order
    for b, p in enumerate(clouds):  # rows past a crop's count are empty
        assert (idx_dev[b, p.shape[0]:] == -1).all() and (val_dev[b, p.shape[0]:] == 0).all()


def _pack(clouds, device):
    pts = torch.as_tensor(np.concatenate(clouds), device=device)
    off = torch.as_tensor(np.concatenate([[0], np.cumsum([c.shape[0] for c in clouds])]).astype(np.int64), device=device)
    return pts, off


def test_grad_build_clouds(device):
    from dpfm_amd import geometry, ops
    clouds = [R.sphere_cap(n, 10 + n) for n in (70, 3, 45)]
    pts, off = _pack(clouds, device)
    frames = geometry.tangent_frames(pts / pts.norm(dim=-1, keepdim=True))  # the sphere's normals
    nbr, _ = ops.knn(pts, off, 70, 30, omit_self=True)
    idx, val = ops.grad_build(pts, off, 70, frames, nbr)
    assert idx.shape == (3, 70, 31) and val.shape == (3, 70, 31, 2) and val.dtype == torch.float64
    fr = frames.cpu().numpy()
    o = off.cpu().numpy()
    tables = [R.cloud_neighbors(c, 30) for c in clouds]
    assert (tables[1][:, 2:] == -1).all()  # the 3-point cloud: 2 neighbours, 28 empty slots
    assert np.array_equal(nbr.cpu().numpy(), np.concatenate(tables))
    _check_rows(idx.cpu().numpy(), val.cpu().numpy(), clouds, [fr[o[b]:o[b + 1]] for b in range(3)], tables)


def _grid_mesh(seed=0):
    rng = np.random.default_rng(seed)
    g = np.arange(5, dtype=np.float64)
    X, Y = np.meshgrid(g, g, indexing="ij")
    verts = np.stack((X.ravel(), Y.ravel(), 0.2 * rng.normal(size=25)), axis=1)
    faces = []
    for i in range(4):
        for j in range(4):
            a, b, c, d = 5 * i + j, 5 * (i + 1) + j, 5 * (i + 1) + j + 1, 5 * i + j + 1
            faces += [[a, b, c], [a, c, d]]
    return verts, np.asarray(faces, np.int32)


def test_grad_build_mesh(device):
    from dpfm_amd import geometry
    verts, faces = _grid_mesh()
    table = R.mesh_neighbors(faces, 25)
    deg = (table >= 0).sum(1)
    assert deg.max() == 6 and deg.min() == 2 and table.shape[1] == 6
    assert np.array_equal(geometry.mesh_neighbor_table([faces], [25]), table)
    pts, off = _pack([verts], device)
    normals = geometry.mesh_vertex_normals(pts, torch.as_tensor(faces.astype(np.int64), device=device))
    frames = geometry.tangent_frames(normals)
    op = geometry.build_grad_operator(pts, off, [25], frames, torch.as_tensor(table, device=device))
    assert op.idx.shape == (1, 25, 7)
    _check_rows(op.idx.cpu().numpy(), op.val.cpu().numpy(), [verts], [frames.cpu().numpy()], [table])


def test_get_operators_fills_grad(device, tmp_path):
    from dpfm_amd import geometry
    from dpfm_amd.dataset.formats import load_operator_npz, save_operator_npz
    clouds = [R.sphere_cap(n, 20 + n) for n in (70, 45)]
    op = geometry.get_operators(clouds, k_eig=8, device=device)
    assert op.grad is not None and op.grad.idx.shape == (2, 70, 31) and op.grad.counts == (70, 45)
    fr, o = op.frames.cpu().numpy(), [0, 70, 115]
    # the operator's table: the 30 nearest neighbours, each row ascending
    tables = [np.sort(R.cloud_neighbors(c, 30), axis=1).astype(np.int32) for c in clouds]
    _check_rows(op.grad.idx.cpu().numpy(), op.grad.val.cpu().numpy(), clouds, [fr[o[b]:o[b + 1]] for b in range(2)],
                tables)
    gx, gy = op.gradX, op.gradY
    assert gx[1].is_sparse and tuple(gx[1].shape) == (45, 45) and tuple(gy[0].shape) == (70, 70)
    # the cache format round-trips the operator of a crop
    path = tmp_path / "ops.npz"
    save_operator_npz(path, {"evecs": op.evecs[1, :45].cpu(), "gradX": gx[1].cpu(), "gradY": gy[1].cpu()})
    got = load_operator_npz(path).data
    assert torch.equal(got["gradX"].to_dense(), gx[1].cpu().to_dense())
    assert torch.equal(got["gradY"].to_dense(), gy[1].cpu().to_dense())
    back = geometry.GradOperator.from_coo([got["gradX"]], [got["gradY"]], nmax=70)
    assert torch.equal(back.idx[0], op.grad.idx[1].cpu()) and torch.equal(back.val[0], op.grad.val[1].cpu())

    verts, faces = _grid_mesh(1)
    mop = geometry.get_operators([verts], [faces], k_eig=8, device=device)
    assert mop.grad is not None and mop.grad.idx.shape == (1, 25, 7) and mop.grad.counts == (25,)
    _check_rows(mop.grad.idx.cpu().numpy(), mop.grad.val.cpu().numpy(), [verts], [mop.frames.cpu().numpy()],
                [R.mesh_neighbors(faces, 25)])
