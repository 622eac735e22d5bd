"""NumPy restatement of the device-side 'random_imp' frame-set draw (include/mocodad_hip.h, mcd_random_imp_masks), written
from the header's description alone: Philox4x32-10 words, multiply-high, r-th frame not chosen yet.  Vectorised over the windows;
every intermediate is uint64 so that nothing wraps except where a `& M32` says so.  Test code only: nothing under mocodad_amd/
imports it."""
import numpy as np

M32 = np.uint64(0xFFFFFFFF)
_MUL0, _MUL1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
_S32 = np.uint64(32)


def philox4x32_10(seed, c0, c1, c2, c3):
    """Four uint32 words (as uint64 arrays, output order) per counter; key = (low, high) 32 bits of `seed`."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & M32 for c in (c0, c1, c2, c3))
    c0, c1, c2, c3 = np.broadcast_arrays(c0, c1, c2, c3)
    seed = int(seed) & (2 ** 64 - 1)
    k0, k1 = np.uint64(seed & 0xFFFFFFFF), np.uint64(seed >> 32)
    for _ in range(10):
        p0, p1 = _MUL0 * c0, _MUL1 * c2           # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> _S32) ^ c1 ^ k0, p1 & M32, (p0 >> _S32) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + _W0) & M32, (k1 + _W1) & M32
    return c0, c1, c2, c3


def masks(seed, first, n, T, k):
    """(n,) int32 bitmasks of the condition frames of windows first .. first + n - 1: exactly k of the bits 0 .. T-1."""
    assert 1 <= k < T <= 32 and n >= 0
    win = (np.arange(n, dtype=np.uint64) + np.uint64(int(first) & (2 ** 64 - 1))) & M32      # the window id wraps at 32 bits
    chosen = np.zeros(n, dtype=np.uint64)
    words = None
    for i in range(k):
        if i % 4 == 0:
            words = philox4x32_10(seed, np.uint64(i // 4), M32, M32, win)
        r = (words[i % 4] * np.uint64(T - i)) >> _S32          # multiply-high: uniform on 0 .. T-i-1
        # the r-th (0-based, ascending) frame not chosen yet
        seen = np.zeros(n, dtype=np.int64)
        pick = np.full(n, -1, dtype=np.int64)
        for t in range(T):
            free = ((chosen >> np.uint64(t)) & np.uint64(1)) == 0
            hit = free & (seen == r.astype(np.int64)) & (pick < 0)
            pick[hit] = t
            seen += free
        assert (pick >= 0).all()
        chosen |= np.uint64(1) << pick.astype(np.uint64)
    return chosen.astype(np.uint32).view(np.int32)
