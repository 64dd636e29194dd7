"""fd_top5_kernel's escape paths on clustered CAD rows (csrc/featdist.hip): the 16-slot candidate
list and its overflow, E3's ranking, E3b's recompute task list and its overflow, E3c's short list
and its overflow, the slow path and the row-part merge (fd_merge_kernel, csrc/featdist.hpp), against
the stable top-5 of the host's
emulation of the same fp32 distances (tests/_util.fd_emulate, exact fmaf). The inputs and the host
model that shows which path each one takes are in tests/_fd_top5_model.py; tests/
test_fd_top5_model_cpu.py checks both without a device. Indices must be equal in every column and
distances bit-equal: with the exact fmaf the emulation leaves no column in doubt."""
import numpy as np
import pytest
import torch

import _fd_top5_model as M

pytestmark = pytest.mark.gpu
V1 = M.V1


def _launch(device, ex, ey, n1, n2):
    """top-5 and top-1 of one batch (C = I): idx5 [B, V2, 5], dist5, idx1 [B, V2, 1], dist1."""
    from dpfm_amd import ops
    B = ex.shape[0]
    C = torch.eye(30).repeat(B, 1, 1).to(device)
    t1 = torch.tensor(n1, dtype=torch.int32, device=device)
    t2 = torch.tensor(n2, dtype=torch.int32, device=device)
    x, y = torch.from_numpy(ex).to(device), torch.from_numpy(ey).to(device)
    i5, d5 = ops.feat_dist_topk(x, C, y, t1, t2, 5, want_dist=True)
    i1, d1 = ops.feat_dist_topk(x, C, y, t1, t2, 1, want_dist=True)
    torch.cuda.synchronize()
    return i5.cpu().numpy(), d5.cpu().numpy(), i1.cpu().numpy(), d1.cpu().numpy()


def _compare(got, b, n2, ei, ev, what):
    """Crop b's n2 columns against the expected indices [n2, 5] and clamped values: zero columns
    may differ, the distances are sqrt of the values bit for bit (inf beside every -1), and the
    top-1 pass returns the first of the five."""
    i5, d5, i1, d1 = got
    bad = np.nonzero((i5[b, :n2] != ei).any(1))[0]
    assert bad.size == 0, (what, b, bad.size, bad[:4], i5[b, bad[:2]], ei[bad[:2]], d5[b, bad[:2]] ** 2, ev[bad[:2]])
    np.testing.assert_array_equal(d5[b, :n2].view(np.int32), np.sqrt(ev).view(np.int32), err_msg=f"{what} crop {b}")
    np.testing.assert_array_equal(i1[b, :n2, 0], ei[:, 0], err_msg=f"{what} crop {b} top-1")
    np.testing.assert_array_equal(d1[b, :n2, 0].view(np.int32), np.sqrt(ev[:, 0]).view(np.int32))


def _tiled(name, n2):
    """A named input's columns repeated up to n2: (ey [n2, 32], d [n1, n2], expected idx, values)
    (a column's distances and its five depend on that column alone)."""
    _, ey, _, p, d, ei, ev = M.case(name)
    j = np.arange(n2) % p
    return ey[j], d[:, j], ei[j], ev[j]


def test_top5_paths_one_part_per_block(device):
    """B = 192 x 128 columns: the smallest batch whose plan is one row part (RS = 1) at 1024 rows,
    with the B % 8 == 0 block mapping. The crops cycle through every input: task-list overflow
    (one base per stream and per stream pair, eps 1e-3 and exact ties, n1 1024 and 1019), the
    16-slot overflow, the short-list merge, the short-list overflow, ties across waves and plain
    random."""
    B, V2 = 192, 128
    assert M.top1_plan(B, V1, V2) == (1, 1) and M.top1_plan(B - 1, V1, V2)[1] > 1
    names = sorted(M.INPUTS)
    ex = np.zeros((B, V1, 32), np.float32)
    ey = np.zeros((B, V2, 32), np.float32)
    n1, n2 = [], []
    for b in range(B):
        x, y, a, c = M.case(names[b % len(names)])[:4]
        ex[b], ey[b, :c] = x, y
        n1.append(a)
        n2.append(c)
    for name in names:  # the path each input takes under this launch's plan
        if name not in M.NO_CONDITIONS:
            M.check_conditions(name, M.top5_block(M.case(name)[4], 1, 0, 0, M.case(name)[3])[1])
    got = _launch(device, ex, ey, n1, n2)
    for b in range(B):
        name = names[b % len(names)]
        _compare(got, b, n2[b], *M.case(name)[5:], name)


def test_top5_paths_column_groups(device):
    """B = 25 x 1000 columns: 8 column groups, 200 blocks, RS = 1 with the B % 8 != 0 block mapping
    and j0 > 0. The overflow and merge inputs' columns are repeated across the groups, n2 ragged (a
    last block of 104 columns still overflows; groups past n2 leave at once); the last crop has 3
    CAD rows: -1 and inf in the fourth and fifth place."""
    B, V2 = 25, 1000
    assert M.top1_plan(B, V1, V2) == (8, 1)
    names = [n for n in sorted(M.INPUTS) if n.startswith(("overflow", "merge"))]
    n2s = [1000, 1000, 640, 897, 1000, 385, 1000, 130, 1000, 999, 513, 768]
    ex = np.zeros((B, V1, 32), np.float32)
    ey = np.zeros((B, V2, 32), np.float32)
    n1, n2, exp = [], [], []
    for b in range(B - 1):
        name, c = names[b % len(names)], n2s[(b + b // len(names)) % len(n2s)]
        y, d, ei, ev = _tiled(name, c)
        ex[b], ey[b, :c] = M.case(name)[0], y
        n1.append(M.case(name)[2])
        n2.append(c)
        exp.append((ei, ev, name))
        if b < len(names) and b % 3 == 0:  # a first, an inner and the last (ragged) block of some crops
            for j0 in {0, 128 * ((c - 1) // 128 // 2), 128 * ((c - 1) // 128)}:
                j1 = min(j0 + 128, c)
                keys, facts = M.top5_block(d, 1, 0, j0, j1)
                np.testing.assert_array_equal((keys & np.uint64(0xFFFFFFFF)).astype(np.int64).T, ei[j0:j1])
                if j1 - j0 >= 100:
                    M.check_conditions(name, facts)
    from _util import fd_emulate, fd_expected_topk
    x, y = M.case("random")[:2]
    ex[B - 1], ey[B - 1, :128] = x, y
    n1.append(3)
    n2.append(128)
    ei, ev = fd_expected_topk(fd_emulate(x, M.EYE, y, 3, 128), 5)
    assert (ei[:, 3:] == -1).all() and np.isinf(ev[:, 3:]).all()
    exp.append((ei, ev, "random, 3 rows"))
    got = _launch(device, ex, ey, n1, n2)
    for b in range(B):
        _compare(got, b, n2[b], *exp[b])


@pytest.mark.parametrize("B", [2, 3])
def test_top5_paths_row_parts(device, B):
    """B = 2 and 3 x 128 columns: RS = 4, two row tiles per wave, and the fd_merge_kernel<5> launch.
    The eps = 0 inputs: within a part a wave's two equal rows list their stream, and the ties_wide
    inputs' equal rows lie in all four parts, fewer than five in each, so the merged five must take
    them from several parts, lowest row first."""
    V2 = 128
    assert M.top1_plan(B, V1, V2) == (1, 4)
    names = ["overflow_tie", "ties_wide"] if B == 2 else ["overflow_pair_tie_1019", "short8_tie_1019", "ties_wide_1019"]
    ex = np.zeros((B, V1, 32), np.float32)
    ey = np.zeros((B, V2, 32), np.float32)
    n1, n2 = [], []
    for b, name in enumerate(names):
        x, y, a, c, d, ei, ev = M.case(name)
        ex[b], ey[b, :c] = x, y
        n1.append(a)
        n2.append(c)
        gi, gv, facts = M.top5_columns(d, 4, 0, c)
        np.testing.assert_array_equal(gi, ei)
        listed = [int(f["nlisted"].sum()) for f in facts]
        assert min(listed) > 0 and sum(int(f["task_total"]) for f in facts) > 0, (name, listed)
        # exact ties across row parts: some column's five hold equal values from different parts
        tie = (ev[:, 1:] == ev[:, :-1]) & (ei[:, 1:] // 256 != ei[:, :-1] // 256)
        assert tie.sum() >= 10 or not name.startswith("ties_wide"), name
    got = _launch(device, ex, ey, n1, n2)
    for b, name in enumerate(names):
        _compare(got, b, n2[b], *M.case(name)[5:], name)
