"""An integer-exact host model of nce_select_kernel (csrc/corr.hip): the keyed pseudo-random
bijection of [0, m), m = min(count, cap), that draws each crop's NCE pair rows.

  key   = splitmix64(seed ^ splitmix64(ctr * 0x100000001B3 + crop))  -> three 32-bit round keys
  perm  = three rounds of (odd multiply + key) mod 2^p and an xor-shift right by ceil(p / 2) on
          [0, 2^p), 2^p the first power of two >= m (p >= 1), cycle-walked until the value is < m
  slot i < min(num, cap) of a crop holds perm(i) when i < m, and (row 0, valid 0) otherwise.

Everything is unsigned integer arithmetic, so the model and the device agree bit for bit or one of
them is wrong. The model restates the kernel round for round, so equality with the device alone
proves nothing about the draw: test_nce_select_cpu.py holds the model to the properties the loss
needs (distinct in-range rows, a permutation at full length, uniform inclusion) and to the
published splitmix64 values. All products stay below 2^64 (a value < 2^32 times a 32-bit constant) or wrap
mod 2^64 as the kernel's do."""
import numpy as np

_M64 = (1 << 64) - 1
_MUL = (0x9E3779B1, 0x85EBCA77, 0xC2B2AE3D)


def splitmix64(x: int) -> int:
    x = (x + 0x9E3779B97F4A7C15) & _M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & _M64
    return x ^ (x >> 31)


def round_keys(seed: int, ctr: int, crop: int):
    h = splitmix64((seed & _M64) ^ splitmix64(((ctr & _M64) * 0x100000001B3 + crop) & _M64))
    return h & 0xFFFFFFFF, h >> 32, splitmix64(h) & 0xFFFFFFFF


def perm_bits(m: int):
    """(p, mask, shift) of the power-of-two domain that holds [0, m)."""
    p = 1
    while (1 << p) < m:
        p += 1
    return p, (1 << p) - 1 if p < 32 else 0xFFFFFFFF, (p + 1) // 2


def perm_step(x: np.ndarray, mask: int, sh: int, keys) -> np.ndarray:
    """One pass of the three rounds on uint64 values below 2^32 (the kernel's uint32 arithmetic:
    the products are reduced by the mask, which is at most 2^32 - 1)."""
    for mul, k in zip(_MUL, keys):
        x = (x * np.uint64(mul) + np.uint64(k)) & np.uint64(mask)
        x = x ^ (x >> np.uint64(sh))
    return x


def select_crop(count: int, cap: int, num: int, seed: int, ctr: int, crop: int):
    """One crop's (rows int64 [k], valid bool [k]), k = min(num, cap)."""
    k = min(num, cap)
    m = max(min(count, cap), 0)
    rows = np.zeros(k, dtype=np.int64)
    valid = np.zeros(k, dtype=bool)
    n = min(k, m)
    if n == 0:
        return rows, valid
    _, mask, sh = perm_bits(m)
    keys = round_keys(seed, ctr, crop)
    y = perm_step(np.arange(n, dtype=np.uint64), mask, sh, keys)
    while True:  # cycle walking: a bijection of [0, 2^p) returns to [0, m) on every cycle that starts there
        out = y >= np.uint64(m)
        if not out.any():
            break
        y[out] = perm_step(y[out], mask, sh, keys)
    rows[:n] = y.astype(np.int64)
    valid[:n] = True
    return rows, valid


def select(counts, cap: int, num: int, seed: int, ctr: int):
    """ops.nce_select on the host: (rows int64 [B, k], valid bool [B, k]) of one call with *ctr = ctr."""
    k = min(num, cap)
    rows = np.zeros((len(counts), k), dtype=np.int64)
    valid = np.zeros((len(counts), k), dtype=bool)
    for b, c in enumerate(counts):
        rows[b], valid[b] = select_crop(int(c), cap, num, seed, ctr, b)
    return rows, valid
