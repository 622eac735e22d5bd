"""CPU: the device-side 'random_imp' frame-set draw as the header fixes it, on its NumPy restatement (tests/rndimp_ref.py) --
check values, bit counts, uniformity over the subsets, per-frame inclusion, independence of neighbouring windows -- plus the
argument checks of mcd_random_imp_masks (made before any device call) and the module's `random_imp_draw` key.
The GPU test (test_random_imp_device_gpu.py) holds the kernel to this restatement bit for bit."""
import ctypes
import itertools
import math

import numpy as np
import pytest
import torch

import rndimp_ref as R
from conftest import load_golden
from helpers import golden_weights, make_args

SEED = 999
P_MIN = 1e-3          # the threshold of tests/test_perf_mode_gpu.py
SHAPES = [(2, 1), (6, 2), (6, 3), (7, 6), (32, 5), (32, 31)]


@pytest.fixture(scope="module")
def drawn():
    """masks(SEED, 0, n, T, k) as uint32, drawn once per (T, k, n) and shared (read-only) by the tests."""
    cache = {}

    def get(T, k, n):
        if (T, k, n) not in cache:
            m = R.masks(SEED, 0, n, T, k).view(np.uint32)
            m.setflags(write=False)
            cache[(T, k, n)] = m
        return cache[(T, k, n)]
    return get


def _popcount(m):
    return np.unpackbits(np.ascontiguousarray(m).view(np.uint8)).reshape(len(m), 32).sum(1)


def test_check_values():
    assert R.masks(999, 0, 3, 6, 3).tolist() == [37, 35, 37]
    # the window id wraps at 32 bits, like the noise key: ids 2^32-3, 2^32-2, 2^32-1, then 0, 1, 2 again
    assert R.masks(999, 2 ** 32 - 3, 6, 6, 3).tolist() == [38, 49, 25, 37, 35, 37]


@pytest.mark.parametrize("T,k", SHAPES)
def test_exactly_k_bits_below_T(drawn, T, k):
    m = drawn(T, k, 1000)
    assert (_popcount(m) == k).all()
    assert (m.astype(np.uint64) >> np.uint64(T) == 0).all()
    if T == 32:       # bit 31 is the int32 sign bit: legal, and it does occur
        assert (m.view(np.int32) < 0).any()


@pytest.mark.parametrize("T,k,n", [(6, 3, 200000), (6, 2, 200000), (7, 6, 70000)])
def test_uniform_over_the_subsets(drawn, T, k, n):
    from scipy.stats import chisquare
    m = drawn(T, k, n)
    subsets = [sum(1 << f for f in c) for c in itertools.combinations(range(T), k)]
    assert len(subsets) == math.comb(T, k)
    counts = np.array([(m == s).sum() for s in subsets])
    assert counts.sum() == n, "a mask that is no k-subset of the T frames"
    assert (counts > 0).all(), "every subset must occur"
    p = chisquare(counts).pvalue
    print(f"T {T} k {k}: {len(subsets)} subsets, chi-square p = {p:.3f}")
    assert p > P_MIN


@pytest.mark.parametrize("T,k,n", [(32, 5, 200000), (32, 31, 50000)])
def test_per_frame_inclusion(drawn, T, k, n):
    m = drawn(T, k, n)
    counts = np.array([((m >> np.uint32(t)) & 1).sum() for t in range(T)], dtype=np.float64)
    q = k / T
    z = (counts - n * q) / math.sqrt(n * q * (1 - q))
    print(f"T {T} k {k}: largest |z| over the frames = {np.abs(z).max():.2f}")
    assert np.abs(z).max() < 4.5


@pytest.mark.parametrize("T,k,n", [(6, 3, 200000), (6, 2, 200000), (32, 5, 200000)])
def test_neighbouring_windows_are_independent(drawn, T, k, n):
    """frame 0 in window b against frame 0 in window b + 1: the counters of neighbours differ in c3 alone"""
    from scipy.stats import chi2_contingency
    f0 = (drawn(T, k, n) & 1).astype(np.int64)
    a, b = f0[:-1], f0[1:]
    table = np.array([[((a == i) & (b == j)).sum() for j in (0, 1)] for i in (0, 1)])
    p = chi2_contingency(table, correction=False)[1]
    print(f"T {T} k {k}: 2x2 table {table.tolist()}, p = {p:.3f}")
    assert p > P_MIN


def test_restatement_rejects_what_the_entry_rejects():
    for T, k in [(6, 0), (6, 6), (33, 5)]:
        with pytest.raises(AssertionError):
            R.masks(1, 0, 4, T, k)


# ---------------------------------------------------------------- the C entry, without a GPU
def _entry():
    from mocodad_amd import _lib
    return _lib.lib()


@pytest.mark.parametrize("seg_len,n_cond,n_windows,names", [
    (6, 0, 4, b"n_cond"), (6, 6, 4, b"n_cond"), (33, 5, 4, b"seg_len"), (6, 3, -1, b"n_windows")])
def test_entry_rejects_bad_arguments_before_any_device_call(seg_len, n_cond, n_windows, names):
    L = _entry()
    buf = (ctypes.c_int32 * 8)()          # (host memory: a call that got as far as a launch would not return MCD_EINVAL)
    rc = L.mcd_random_imp_masks(ctypes.c_uint64(1), ctypes.c_int64(0), n_windows, seg_len, n_cond, buf, None)
    assert rc == -1          # MCD_EINVAL
    assert names in L.mcd_last_error()


def test_entry_accepts_zero_windows():
    L = _entry()
    assert L.mcd_random_imp_masks(ctypes.c_uint64(1), ctypes.c_int64(0), 0, 6, 3, None, None) == 0


def test_aggregate_view_refuses_a_strided_view_without_a_gpu():
    from mocodad_amd import _lib
    L = _entry()
    cfg = _lib.ScoreCfg(n_windows=2, n_samples=2, noise_steps=3, seg_len=6, n_cond=2, n_corrupt=4, loss_fn=0)
    buf = (ctypes.c_float * 8)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    view = _lib.WindowView(base=p, stride_c=17, stride_t=34, trans=None, affine=None, cond_mask=None)
    rc = L.mcd_aggregate_view(ctypes.byref(cfg), 2, 17, _lib.AGGR["best"], ctypes.c_float(0), p, None, None, ctypes.byref(view), p, None, None)
    assert rc == -1 and b"base" in L.mcd_last_error()


# ---------------------------------------------------------------- the module key
def test_module_key_random_imp_draw():
    from mocodad_amd.models.mocodad import MoCoDAD
    _, cfg = golden_weights("rndimp")
    assert "random_imp_draw" not in cfg
    m = MoCoDAD(make_args(cfg))
    assert m.random_imp_draw == "host"                      # the key is absent: the reference's draw
    assert MoCoDAD(make_args(cfg, random_imp_draw="host")).random_imp_draw == "host"
    assert MoCoDAD(make_args(cfg, random_imp_draw="device")).random_imp_draw == "device"
    with pytest.raises(ValueError, match="random_imp_draw"):
        MoCoDAD(make_args(cfg, random_imp_draw="bogus"))
    # 'host' is the code it was: the fixture's sets under the fixture's seed
    g = load_golden("traj_rndimp_ns4_S2.npz")
    for mod in (m, MoCoDAD(make_args(cfg, random_imp_draw="host"))):
        torch.manual_seed(int(g["rng_seed"][0]))
        assert torch.equal(mod.draw_random_imp_mask(g["data"].shape[0]), torch.from_numpy(g["cond_mask"]))
