"""A host model of fd_top5_kernel's selection (csrc/featdist.hip), and the clustered inputs that
drive its escape paths.

The model takes one crop's emulated distances (tests/_util.fd_emulate: the kernel's own fp32 bits)
and replays, for one block = (row part rs, 128 columns), what the kernel does with them: the
per-stream minimum / tile / second value of the fast path, E1's threshold, E2's candidate list and
its 16 slots, E3's ranking and stream listing, E3b's recompute tasks, E3c's short list, the slow
path, and the row-part merge. All comparisons are the kernel's: signed int32 on the value bits in
the row loop and against the clamp, unsigned (value bits, row) keys in the lists. It returns the
five of every column and the path facts (how many candidates, listed streams, tasks, rows below
the fifth key, and why a column went to the slow path), so that a test can show that an input
reaches the path it was built for before it is sent to the device.

Where LDS atomics leave the order free on the device (which streams reserve their task slots
before the list is full), the model flags every column of an overflowing block slow. The five do
not depend on that: the slow path and the list path produce the same five.
"""
import functools

import numpy as np

K_CLAMP_BITS = 0x0DA24260  # kClampBits: 1e-30f
INF_BITS = 0x7F800000
NO_TILE = 0x07FFFFFF
K_WAVES = 8      # kTop1Waves
K_CT = 8         # kTop1CT: 16-column tiles per block
NC = 16 * K_CT   # columns per block
K_SLOTS = 16     # kT5Slots
K_TASKS = 1536   # kT5Tasks
K_X = 8          # kT5X
NONE_KEY = np.uint64(0xFFFFFFFFFFFFFFFF)


def top1_plan(B, V1max, V2max):
    """(NCG, RS) of a mode-0 top-1 / top-5 launch: top1_plan in csrc/featdist.hip."""
    T1, T2 = (V1max + 15) // 16, (V2max + 15) // 16
    ncg = max(1, -(-T2 // K_CT))
    blocks = B * ncg
    rs = 1 if blocks >= 192 else -(-256 // blocks)
    return ncg, max(1, min(rs, T1 // (2 * K_WAVES)))


def wave_tiles(n1, RS):
    """The row-tile range [tb, te) of each of the Q = 8 RS waves (qw = 8 rs + w): top1_wave_tiles in
    csrc/featdist.hip."""
    nt, Q = (n1 + 15) // 16, K_WAVES * RS
    return [(nt * qw // Q, nt * (qw + 1) // Q) for qw in range(Q)]


def _first5(keys):
    """The five smallest of each column of keys [m, nc] (uint64), ascending."""
    if keys.shape[0] < 5:
        keys = np.concatenate([keys, np.full((5 - keys.shape[0], keys.shape[1]), NONE_KEY)])
    return np.sort(keys, axis=0)[:5]


def top5_block(d, RS, rs, j0, j1):
    """One block: row part rs of RS, columns [j0, j1) (j1 - j0 <= 128, all below the crop's n2) of
    the emulated distances d [n1, n2] (float32). Returns (keys [5, nc] uint64 = value bits << 32 |
    row, ~0 where there is no row; the values are clamped in slow columns only, as the kernel emits
    them) and the facts: per column `ncand`, `cand_clamped` (a candidate stream's minimum is at or
    below the clamp, whatever the column's reason), `nlisted`, `ntask`, `nbelow`, `reason` (None,
    'list16', 'clamp', 'task_clamp', 'short8', 'taskfull': the first that applies, in the kernel's
    order); per block `task_total`."""
    d = np.ascontiguousarray(d[:, j0:j1], dtype=np.float32)
    n1, nc = d.shape
    nt = (n1 + 15) // 16
    K = np.full((nt * 16, nc), INF_BITS, np.int32)  # padding rows are +inf
    K[:n1] = d.view(np.int32)
    rows = np.arange(nt * 16, dtype=np.uint64)[:, None]
    key = (K.view(np.uint32).astype(np.uint64) << np.uint64(32)) | rows
    K3 = K.reshape(nt, 16, nc)
    tiles = wave_tiles(n1, RS)[K_WAVES * rs:K_WAVES * (rs + 1)]
    # the fast path's per-stream state: stream (w, i) = rows 16 t + i over wave w's tiles
    k1 = np.full((K_WAVES, 16, nc), INF_BITS, np.int32)
    k2 = np.full((K_WAVES, 16, nc), INF_BITS, np.int32)
    t1 = np.full((K_WAVES, 16, nc), NO_TILE, np.int64)
    for w, (tb, te) in enumerate(tiles):
        if tb >= te:
            continue
        seg = K3[tb:te]
        k1[w] = seg.min(0)
        # strict <: the first tile that reaches the minimum; +inf never replaces the initial +inf
        t1[w] = np.where(k1[w] < INF_BITS, tb + seg.argmin(0), NO_TILE)
        if te - tb >= 2:  # v_med3 keeps the second smallest of the multiset (an equal key counts)
            k2[w] = np.sort(seg, axis=0)[1]
    # E0/E1: T = the 5th smallest of the 32 lane minima (min over r, i = 4 g + r)
    lm = k1.reshape(K_WAVES, 4, 4, nc).min(2).reshape(4 * K_WAVES, nc)
    T = np.sort(lm, axis=0)[4]
    # E2: the candidate streams
    cand = k1 <= T[None, None]
    ncand = cand.sum((0, 1))
    i_of = np.arange(16)[None, :, None]
    srow = (t1 * 16 + i_of).astype(np.uint64) & np.uint64(0xFFFFFFFF)
    skey = (k1.view(np.uint32).astype(np.uint64) << np.uint64(32)) | srow
    reason = np.full(nc, None, object)
    reason[ncand > K_SLOTS] = "list16"
    clamp = (cand & (k1 <= K_CLAMP_BITS)).any((0, 1))
    reason[(ncand <= K_SLOTS) & clamp] = "clamp"
    # E3: ranks by (value, row) among the candidates with a row; the five and their streams
    ranked = np.where(cand & (k1 < INF_BITS), skey, NONE_KEY).reshape(K_WAVES * 16, nc)
    order = np.argsort(ranked, axis=0, kind="stable")[:5]
    best = np.take_along_axis(ranked, order, 0)  # [5, nc]
    fifth = best[4]
    S = np.where(fifth == NONE_KEY, INF_BITS, (fifth >> np.uint64(32)).astype(np.uint32).view(np.int32))
    # kept streams of ranks 0..3 whose second value is <= the fifth value are listed
    k2f = k2.reshape(K_WAVES * 16, nc)
    listed = np.zeros((K_WAVES * 16, nc), bool)
    fast = np.array([r is None for r in reason])
    for q in range(4):
        st = order[q]
        on = fast & (best[q] != NONE_KEY) & (np.take_along_axis(k2f, st[None], 0)[0] <= S)
        listed[st[on], np.nonzero(on)[0]] = True
    listed = listed.reshape(K_WAVES, 16, nc)
    # E3b's tasks: the listed streams' rows that exist, but the kept one
    task = np.zeros((nt, 16, nc), bool)
    for w, (tb, te) in enumerate(tiles):
        if tb < te:
            task[tb:te] = listed[w][None] & (np.arange(tb, te)[:, None, None] != t1[w][None])
    task = task.reshape(nt * 16, nc) & (np.arange(nt * 16) < n1)[:, None]
    ntask = task.sum(0)
    nlisted = listed.sum((0, 1))
    task_total = int(ntask.sum())
    if task_total > K_TASKS:
        reason[fast] = "taskfull"
        fast[:] = False
    task_clamp = (task & (K <= K_CLAMP_BITS)).any(0)
    below = task & (K > K_CLAMP_BITS) & (key < fifth[None])
    nbelow = below.sum(0)
    reason[fast & task_clamp] = "task_clamp"
    reason[fast & ~task_clamp & (nbelow > K_X)] = "short8"
    # E3c: the short list merged into the five
    out = _first5(np.concatenate([best, np.where(below, key, NONE_KEY)]))
    # the slow path: every row of the part, clamped, lower row first
    slow = np.array([r is not None for r in reason])
    if slow.any():
        r0, r1 = tiles[0][0] * 16, min(tiles[-1][1] * 16, n1)
        Ks = K[r0:r1][:, slow]
        v = np.where(Ks <= K_CLAMP_BITS, K_CLAMP_BITS, Ks).view(np.uint32).astype(np.uint64)
        out[:, slow] = _first5((v << np.uint64(32)) | rows[r0:r1])
    facts = dict(ncand=ncand, cand_clamped=clamp, nlisted=nlisted, ntask=ntask, nbelow=nbelow, reason=reason,
                 task_total=task_total)
    return out, facts


def top5_columns(d, RS, j0, j1):
    """Columns [j0, j1) of one crop through every row part and fd_merge_kernel<5> (the parts' lists
    in row order, merged by value, ties to the earlier entry = the lower row). Returns (idx [nc, 5]
    int64, -1 where there is no row; values [nc, 5] float32, inf there; the facts of each part)."""
    parts, facts = [], []
    for rs in range(RS):
        k, f = top5_block(d, RS, rs, j0, j1)
        parts.append(k)
        facts.append(f)
    keys = np.concatenate(parts)  # [5 RS, nc]
    if RS > 1:
        val = (keys >> np.uint64(32)).astype(np.uint32).view(np.float32)
        val = np.where(keys == NONE_KEY, np.float32(np.inf), val)
        o = np.argsort(val, axis=0, kind="stable")[:5]
        keys = np.take_along_axis(keys, o, 0)
    none = keys == NONE_KEY
    idx = np.where(none, -1, (keys & np.uint64(0xFFFFFFFF)).astype(np.int64))
    val = np.where(none, np.float32(np.inf), (keys >> np.uint64(32)).astype(np.uint32).view(np.float32))
    return idx.T.copy(), val.T.astype(np.float32), facts


def top5_crop(d, RS):
    """Every 128-column block of a crop: (idx [n2, 5], values [n2, 5], facts[cg][rs])."""
    n2 = d.shape[1]
    res = [top5_columns(d, RS, j0, min(j0 + NC, n2)) for j0 in range(0, n2, NC)]
    return np.concatenate([r[0] for r in res]), np.concatenate([r[1] for r in res]), [r[2] for r in res]


# ---------------------------------------------------------------------------------------------
# Inputs. V1max = 1024, C = I, 32-wide randn features. Stream (w, i) = rows 16 t + i for t in wave
# w's tile range at RS = 1 (8 tiles at 64 row tiles). The rows past n1 are built too and ignored.
V1 = 1024


def _streams(rng, group, eps):
    """[1024, 32]: every row = its stream's base + eps noise. group = 1: one base per stream; 2: per
    pair of streams i, i ^ 1; 4: per lane, streams 4 g .. 4 g + 3."""
    t = np.arange(V1) // 16
    w, i = t // 8, np.arange(V1) % 16
    base = rng.standard_normal((K_WAVES, 16 // group, 32)).astype(np.float32)
    ex = base[w, i // group]
    return (ex + np.float32(eps) * rng.standard_normal((V1, 32)).astype(np.float32)).astype(np.float32)


def build_overflow(seed, eps, n1, pair=False, n2=128):
    """Every stream clustered: each column lists its four streams, 7 tasks each."""
    rng = np.random.default_rng(seed)
    return _streams(rng, 2 if pair else 1, eps), rng.standard_normal((n2, 32)).astype(np.float32), n1, n2


def build_list16(seed, n1=1024, n2=128):
    """The four streams of a lane share a base: the four lanes below T hold 16 candidates and the
    lane at T adds its minimum (15..17 per column, 126 of 128 columns above 16)."""
    rng = np.random.default_rng(seed)
    return _streams(rng, 4, 1e-3), rng.standard_normal((n2, 32)).astype(np.float32), n1, n2


def build_merge(seed, eps, n1, n2, wide=False):
    """In each stream 2..4 of the 8 tiles are near-copies of one base and the rest are random: where
    a column's nearest rows are copies, its listed streams put their other copies below its fifth
    key (up to 12 rows; the seeds in INPUTS keep every column within the 8-entry short list, and
    one seed fills it exactly. More copies per stream would overflow it: that is build_short8).
    wide: waves w and w + 2, + 4, + 6 share their bases, so with eps = 0 a base's equal rows lie in
    all four row parts of an RS = 4 launch, fewer than five of them in each."""
    rng = np.random.default_rng(seed)
    ex = rng.standard_normal((V1, 32)).astype(np.float32)
    base = rng.standard_normal((K_WAVES, 16, 32)).astype(np.float32)
    for w in range(K_WAVES):
        for i in range(16):
            for t in rng.choice(8, size=rng.integers(2, 5), replace=False):
                row = (8 * w + t) * 16 + i
                ex[row] = base[w % 2 if wide else w, i] + np.float32(eps) * rng.standard_normal(32).astype(np.float32)
    return ex, rng.standard_normal((n2, 32)).astype(np.float32), n1, n2


def build_short8(seed, eps=1e-3, n1=1024):
    """build_overflow at 16 columns: 448 tasks fit the list, 28 rows per column below its fifth."""
    return build_overflow(seed, eps, n1, n2=16)


def build_random(seed, n1=1024, n2=128):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((V1, 32)).astype(np.float32), rng.standard_normal((n2, 32)).astype(np.float32),
            n1, n2)


# name -> (builder, arguments); the GPU tests and the CPU tests draw from this one table
INPUTS = {
    "overflow_eps": (build_overflow, (11, 1e-3, 1024)),
    "overflow_eps_1019": (build_overflow, (12, 1e-3, 1019)),
    "overflow_tie": (build_overflow, (13, 0.0, 1024)),
    "overflow_tie_1019": (build_overflow, (14, 0.0, 1019)),
    "overflow_pair_eps": (build_overflow, (15, 1e-3, 1024, True)),
    "overflow_pair_eps_1019": (build_overflow, (16, 1e-3, 1019, True)),
    "overflow_pair_tie": (build_overflow, (17, 0.0, 1024, True)),
    "overflow_pair_tie_1019": (build_overflow, (18, 0.0, 1019, True)),
    "list16": (build_list16, (21,)),
    "merge_eps": (build_merge, (34, 1e-3, 1024, 48)),
    "merge_eps_1019": (build_merge, (30, 1e-3, 1019, 40)),
    "merge_tie": (build_merge, (40, 0.0, 1024, 44)),
    "merge_tie_1019": (build_merge, (34, 0.0, 1019, 47)),
    "ties_wide": (build_merge, (35, 0.0, 1024, 128, True)),
    "ties_wide_1019": (build_merge, (36, 0.0, 1019, 77, True)),
    "short8": (build_short8, (41,)),
    "short8_tie_1019": (build_short8, (42, 0.0, 1019)),
    "random": (build_random, (51,)),
}
NO_CONDITIONS = ("random", "ties_wide", "ties_wide_1019")  # inputs with no path condition at RS = 1
EYE = np.eye(30, dtype=np.float32)


@functools.lru_cache(maxsize=None)
def case(name):
    """(ex [1024, 32], ey [n2, 32], n1, n2, d = fd_emulate [n1, n2], expected idx, expected clamped
    values) of a named input, computed once per process; treat the arrays as read-only."""
    from _util import fd_emulate, fd_expected_topk
    fn, args = INPUTS[name]
    ex, ey, n1, n2 = fn(*args)
    d = fd_emulate(ex, EYE, ey, n1, n2)
    ei, ev = fd_expected_topk(d, 5)
    for a in (ex, ey, d, ei, ev):
        a.setflags(write=False)
    return ex, ey, n1, n2, d, ei, ev


@functools.lru_cache(maxsize=None)
def crop_result(name, RS):
    """top5_crop of a named input's distances at RS row parts, computed once per process."""
    return top5_crop(case(name)[4], RS)


def check_conditions(name, facts):
    """The conditions an input's path facts must meet for one block at RS = 1 (the issue's section
    3); raises AssertionError naming the figures."""
    ncand, reason, nbelow, total = facts["ncand"], facts["reason"], facts["nbelow"], facts["task_total"]
    clamped = facts["cand_clamped"]
    nc = len(ncand)
    if name.startswith("overflow"):
        assert total > K_TASKS, (name, total)
        assert not clamped.any(), (name, np.nonzero(clamped)[0])
        assert ncand.max() <= K_SLOTS and all(r == "taskfull" for r in reason), (name, ncand.max(), set(reason))
    elif name.startswith("list16"):
        over = ncand > K_SLOTS
        assert over.sum() >= 100 * nc // NC, (name, int(over.sum()))
        assert not clamped[over].any(), (name, np.nonzero(clamped & over)[0])
        assert all(r == "list16" for r in reason[over]), (name, set(reason[over]))
    elif name.startswith("merge"):
        assert total <= K_TASKS, (name, total)
        assert all(r is None for r in reason), (name, set(reason))
        assert ((nbelow >= 1) & (nbelow <= K_X)).sum() >= min(10, nc), (name, nbelow)
    elif name.startswith("short8"):
        assert total <= K_TASKS, (name, total)
        assert (nbelow > K_X).all() and all(r == "short8" for r in reason), (name, nbelow, set(reason))
    else:
        raise KeyError(name)
