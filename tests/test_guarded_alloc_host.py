"""CPU: the guarded-allocation helper of tests/guarded.py, in its CPU mode (guard_cpu=True: CPU results are carved out of a backing
tensor as device results are on the GPU).  What the proxy hands out is what torch hands out; a store of one element before,
right behind and GUARD - 1 bytes behind the interior is reported with its allocation and offset; `unwritten` counts the all-ones
pattern and nothing else; the real torch is back on the two patched modules afterwards."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guarded as G  # noqa: E402

CALLS = [
    ("empty", lambda t: t.empty(3, 5, dtype=torch.float32)),
    ("empty", lambda t: t.empty((2, 3, 2, 7, 17), dtype=torch.float32)),
    ("empty", lambda t: t.empty(1, dtype=torch.int64)),
    ("empty", lambda t: t.empty(7, dtype=torch.float64)),
    ("empty", lambda t: t.empty(2, 32, 17, 2, dtype=torch.float32)),       # a leading-index row of 4352 bytes: more than GUARD
    ("empty", lambda t: t.empty(1000, dtype=torch.uint8)),
    ("zeros", lambda t: t.zeros(4 * 2 * 8 * 34, dtype=torch.float32)),
    ("zeros", lambda t: t.zeros((2, 5, 9), dtype=torch.float64)),
    ("zeros", lambda t: t.zeros(3, 2, 6, dtype=torch.int32)),
    ("full", lambda t: t.full((3,), -7.0)),
    ("full", lambda t: t.full((5, 2), 3, dtype=torch.int32)),
    ("empty_like", lambda t: t.empty_like(torch.ones(5, 2, 3, 17))),
    ("empty_like", lambda t: t.empty_like(torch.ones(4, 32, dtype=torch.float64))),
]


@pytest.mark.parametrize("i", range(len(CALLS)))
def test_the_proxy_hands_out_what_torch_hands_out(i):
    fn, call = CALLS[i]
    g = G.GuardedTorch(guard_cpu=True)
    got, want = call(g), call(torch)
    assert got.shape == want.shape and got.dtype == want.dtype and got.stride() == want.stride() and got.device == want.device
    assert got.is_contiguous()
    e = g.registry[-1]
    assert len(g.registry) == 1 and e["fn"] == fn and e["shape"] == tuple(want.shape) and e["dtype"] == want.dtype
    assert e["nbytes"] == want.numel() * want.element_size()
    # the interior starts a multiple of 256 bytes into the backing block: it keeps the allocator's alignment
    off = got.data_ptr() - e["backing"].data_ptr()
    assert off == e["guard"] and off % 256 == 0 and off >= G.GUARD
    row = want.element_size() * (want.numel() // want.shape[0])
    assert e["guard"] >= row, "the guard is at least one leading-index row"
    assert e["backing"].numel() == 2 * e["guard"] + e["nbytes"]
    if fn in ("zeros", "full"):
        assert torch.equal(got, want)
        assert G.unwritten(got) == 0
    else:
        assert G.unwritten(got) == got.numel()
    assert bool((e["backing"][:off] == G.GUARD_BYTE).all()) and bool((e["backing"][off + e["nbytes"]:] == G.GUARD_BYTE).all())
    assert os.path.basename(__file__) in e["where"]
    g.check()


def test_everything_else_is_forwarded_and_untouched_results_pass_through():
    g = G.GuardedTorch()          # the device mode: CPU and pinned results are torch's own
    assert g.float32 is torch.float32 and g.cuda is torch.cuda and g.Tensor is torch.Tensor and g.is_tensor(torch.ones(1))
    t = g.empty(5, dtype=torch.int32)
    z = g.zeros(2, 3)
    assert not g.registry and t.shape == (5,) and torch.equal(z, torch.zeros(2, 3))
    g = G.GuardedTorch(guard_cpu=True)
    assert g.empty(0, 3).shape == (0, 3) and g.full((0,), 1.0).numel() == 0 and not g.registry        # (nothing to guard)


def _three(g):
    a = g.empty(4, 6, dtype=torch.float32)
    b = g.empty(5, dtype=torch.float64)
    c = g.zeros(3, 2, dtype=torch.int32)
    return a, b, c


def _one_violation(g):
    v = g.violations()
    assert len(v) == 1
    with pytest.raises(G.GuardViolation) as ei:
        g.check()
    return v[0], str(ei.value)


def _past(e, byte_offset):
    """A float32 element written at byte_offset from the interior's first byte (negative: before it), through the backing tensor."""
    at = e["guard"] + byte_offset
    e["backing"][at:at + 4].view(torch.float32)[0] = 1.5        # bytes 00 00 c0 3f


def test_a_write_of_one_element_before_the_interior_is_reported():
    g = G.GuardedTorch(guard_cpu=True)
    a, b, c = _three(g)
    a.fill_(1.0), b.fill_(2.0)
    g.check()
    _past(g.registry[0], -4)
    (name, side, first, last, found, count), text = _one_violation(g)
    assert name == g.allocations()[0] and "empty (4, 6) float32" in name and "_three" in name
    assert (side, first, last, found, count) == ("head", -4, -1, (0x00, 0x3F), 4)
    assert name in text and "head guard" in text and "-4 .. -1" in text and "0x00 .. 0x3f" in text


def test_a_write_of_one_element_behind_the_interior_is_reported():
    g = G.GuardedTorch(guard_cpu=True)
    a, b, c = _three(g)
    e = g.registry[1]
    e["backing"][e["guard"] + e["nbytes"]:].view(torch.float64)[0] = 1.0      # element b[5]: bytes 00 .. 00 f0 3f
    (name, side, first, last, found, count), text = _one_violation(g)
    assert name == g.allocations()[1] and "empty (5,) float64" in name
    assert (side, first, last, found, count) == ("tail", 0, 7, (0x00, 0x3F), 8)
    assert name in text and "tail guard" in text and "0 .. 7" in text


def test_a_write_guard_minus_one_bytes_away_is_reported():
    g = G.GuardedTorch(guard_cpu=True)
    a, b, c = _three(g)
    assert g.registry[0]["guard"] == g.registry[2]["guard"] == G.GUARD
    e = g.registry[2]
    e["backing"][e["guard"] + e["nbytes"] + G.GUARD - 1] = 0x11                # the last byte of the tail guard
    (name, side, first, last, found, count), text = _one_violation(g)
    assert name == g.allocations()[2] and "zeros (3, 2) int32" in name
    assert (side, first, last, found, count) == ("tail", G.GUARD - 1, G.GUARD - 1, (0x11, 0x11), 1)
    e = g.registry[0]
    e["backing"][0] = 0x22                                                      # the first byte of the head guard
    v = g.violations()
    assert len(v) == 2 and v[0][:5] == (g.allocations()[0], "head", -G.GUARD, -G.GUARD, (0x22, 0x22))


def test_a_short_interior_puts_the_last_row_into_the_tail_guard():
    g = G.GuardedTorch(guard_cpu=True, short_rows=1)
    t = g.empty(5, 2, 17, dtype=torch.float32)
    e = g.registry[0]
    assert t.shape == (5, 2, 17) and e["nbytes"] == 4 * 136 and e["backing"].numel() == 2 * e["guard"] + 4 * 136
    t[:4] = 1.0
    g.check()
    t[4] = 1.0              # the legitimate last row: inside the backing tensor, outside the registered interior
    (name, side, first, last, found, count), _ = _one_violation(g)
    assert (side, first, last, count) == ("tail", 0, 135, 136)


def test_unwritten_counts_the_all_ones_pattern_only():
    g = G.GuardedTorch(guard_cpu=True)
    t = g.empty(3, 4, dtype=torch.float32)
    assert G.unwritten(t) == 12
    t[0] = 0.5
    t[1, 0] = float("nan")                                          # torch's canonical NaN 0x7fc00000
    t.view(torch.int32)[1, 1] = 0x7FC00000
    t.view(torch.int32)[1, 2] = -4194304                            # 0xffc00000: a NaN with the sign set, still not all ones
    assert G.unwritten(t) == 12 - 4 - 3
    d = g.empty(4, dtype=torch.float64)
    d[1] = float("nan")
    d[2] = 0.0
    assert G.unwritten(d) == 2
    i = g.empty(6, dtype=torch.int64)
    i[:5] = torch.arange(5)
    assert G.unwritten(i) == 1
    assert G.unwritten(g.zeros(4)) == 0 and G.unwritten(torch.empty(0)) == 0


@pytest.mark.parametrize("fill", ["nan", "finite"])
def test_guarded_copy_holds_the_tensor_between_two_bands(fill):
    t = torch.randn(3, 2, 6, 17, generator=torch.Generator().manual_seed(1))
    c = G.guarded_copy(t, fill)
    assert torch.equal(c, t) and c.shape == t.shape and c.is_contiguous() and c.data_ptr() % 16 == 0
    store = torch.empty(0, dtype=torch.float32).set_(c.untyped_storage())
    n, g = t.numel(), G.GUARD // 4
    assert store.numel() == n + 2 * g and c.storage_offset() == g
    bands = torch.cat([store[:g], store[g + n:]])
    if fill == "nan":
        assert bool((bands.view(torch.int32) == -1).all())
    else:
        assert bool(torch.isfinite(bands).all()) and bool((bands.abs() < 1).all()) and bands.unique().numel() > g
    with pytest.raises(ValueError):
        G.guarded_copy(t, "zeros")


def test_the_real_torch_is_back_after_the_context():
    import mocodad_amd.engine as engine
    import mocodad_amd.stream as stream
    assert engine.torch is torch and stream.torch is torch
    with G.guarded() as g:
        assert engine.torch is g and stream.torch is g and isinstance(g, G.GuardedTorch)
        import mocodad_amd.parallel as parallel
        assert parallel.torch is torch, "only the two allocating modules see the proxy"
    assert engine.torch is torch and stream.torch is torch
    with pytest.raises(RuntimeError, match="inside"):
        with G.guarded(short_rows=1) as g:
            assert engine.torch is g and g._short_rows == 1
            raise RuntimeError("inside")
    assert engine.torch is torch and stream.torch is torch
