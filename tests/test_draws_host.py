"""CPU: the NumPy restatement of the noise draws (tests/draws_ref.py) -- Philox known answers, the restatement's own sanity, and
the sharpness of the gate tests/test_draws_gpu.py puts on the exported tensors: close_draws rejects every single-field mistake of
draws_ref.MISTAKES at every shape tried, so a kernel that made one of them could not pass it.  The last test holds the GPU
module's case table against the kernel rows of csrc/mcd_instances.hpp."""
import os
import re

import numpy as np
import pytest

import draws_ref as D
from rndimp_ref import philox4x32_10

SEED = 0xFEDCBA9876543210
WRAP = 2 ** 32 - 2              # first_window_id: the id wraps inside a batch of 5


# Random123's known-answer vectors of philox4x32-10 (kat_vectors): counter, key, output words
KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


@pytest.mark.parametrize("ctr,key,words", KAT, ids=["zeros", "ones", "pi"])
def test_philox_known_answers(ctr, key, words):
    got = philox4x32_10(key[0] | (key[1] << 32), *ctr)
    assert tuple(int(w) for w in got) == words


def test_uniform_is_float32_and_its_ends():
    u = D.uniform(np.array([0, 0xFF, 0x100, 0x7FFFFFFF, 0xFFFFFEFF, 0xFFFFFFFF], dtype=np.uint64))
    assert u.dtype == np.float32
    assert u[0] == u[1] == np.float32(2.0 ** -25) and u[2] == np.float32(1.5 * 2.0 ** -24)
    assert u[3] == np.float32((2.0 ** 23 - 0.5) * 2.0 ** -24)      # 2^23 - 1 + 0.5 needs 24 bits: exact
    assert u[4] == np.float32(1.0 - 2.0 ** -23)         # 2^24 - 2 + 0.5 ties to the even neighbour
    assert u[5] == np.float32(1.0)                      # the largest word: 2^24 - 1 + 0.5 rounds up
    z = D.box_muller(np.array([0xFFFFFFFF], dtype=np.uint64), np.array([12345], dtype=np.uint64))
    assert z[0][0] == 0.0 and z[1][0] == 0.0            # ... and gives r = 0


def _rows(words):
    return np.stack([np.asarray(w, dtype=np.uint64).reshape(-1) for w in words], axis=1)


@pytest.mark.parametrize("kind", ["pose", "latent"])
def test_restatement_sanity(kind):
    """Tx 32 (D 128), S 3, ns 4, B 5, the window id wrapping inside the batch: no two calls share a counter or their words, every
    value is finite and inside Box-Muller's range, mean and variance within 4 standard errors."""
    S, ns, B = 3, 4, 5
    if kind == "pose":
        calls, z = D.pose_calls(SEED, WRAP, B, S, ns, 32), D.pose_noise(SEED, WRAP, B, S, ns, 32)
        assert z.shape == (S, 3, B, 2, 32, 17)
        assert sum(c[0][0].size for c in calls) == S * B * 2 * 32 * 17 + S * 2 * B * 32 * 9
    else:
        calls, z = D.latent_calls(SEED, WRAP, B, S, ns, 128), D.latent_noise(SEED, WRAP, B, S, ns, 128)
        assert z.shape == (S, 3, B, 128)
        assert sum(c[0][0].size for c in calls) == S * 3 * B * 32
    ctr = np.concatenate([_rows(c) for c, _ in calls])
    words = np.concatenate([_rows(w) for _, w in calls])
    assert np.unique(ctr, axis=0).shape[0] == ctr.shape[0], "two calls share a counter"
    assert np.unique(words, axis=0).shape[0] == words.shape[0], "two calls share their words"
    assert set(np.unique(ctr[:, 3]).tolist()) == {2 ** 32 - 2, 2 ** 32 - 1, 0, 1, 2}
    assert z.dtype == np.float64 and not np.isnan(z).any()
    assert np.abs(z).max() < 5.9                        # sqrt(2 * 25 * ln 2) = 5.887: u >= 2^-25
    n = z.size
    assert abs(z.mean()) < 4 / np.sqrt(n) and abs(z.var() - 1) < 4 * np.sqrt(2 / n), (z.mean(), z.var(), n)
    # the slots and samples of one window are different draws, and the same keys reproduce
    again = D.pose_noise(SEED, WRAP, B, S, ns, 32) if kind == "pose" else D.latent_noise(SEED, WRAP, B, S, ns, 128)
    assert np.array_equal(z, again)
    assert D.close_draws(z, z) == (True, 0.0, (0,) * z.ndim)


def test_slot_count_and_window_ids():
    assert [D.n_slots(ns) for ns in (2, 3, 4, 10)] == [1, 2, 3, 9]
    assert D.pose_noise(SEED, 0, 2, 2, 2, 3).shape == (2, 1, 2, 2, 3, 17) and D.latent_noise(SEED, 0, 2, 2, 2, 16).shape == (2, 1, 2, 16)
    assert D.window_ids(-3, 5).tolist() == [2 ** 32 - 3, 2 ** 32 - 2, 2 ** 32 - 1, 0, 1]
    assert D.window_ids(2 ** 40 + 5, 2).tolist() == [5, 6]
    # a batch is a slice of a longer one: windows keep their draws wherever the call starts
    a, b = D.pose_noise(SEED, 7, 5, 2, 3, 2), D.pose_noise(SEED, 9, 3, 2, 3, 2)
    assert np.array_equal(a[:, :, 2:], b)


SHARP = [(w, k, n) for w, kinds in D.MISTAKES.items() for k, n in (("pose", 3), ("pose", 13), ("latent", 16), ("latent", 48)) if k in kinds]


def test_the_list_of_mistakes():
    assert len(D.MISTAKES) == 10 and len(SHARP) == 7 * 4 + 3 * 2
    assert {w for w, k in D.MISTAKES.items() if k == ("pose",)} == {"xT_Tx+1", "step_tx*8"}
    assert {w for w, k in D.MISTAKES.items() if k == ("latent",)} == {"latent_d0/8"}


@pytest.mark.parametrize("wrong,kind,size", SHARP, ids=[f"{w}-{k}{n}" for w, k, n in SHARP])
def test_the_gate_rejects_every_single_field_mistake(wrong, kind, size):
    """S 3, ns 4, B 5, window ids wrapping inside the batch: the restatement with one field wrong does not pass close_draws
    against the restatement, and misses it on at least 17 elements."""
    fn = D.pose_noise if kind == "pose" else D.latent_noise
    ref = fn(SEED, WRAP, 5, 3, 4, size)
    bad = fn(SEED, WRAP, 5, 3, 4, size, wrong=wrong)
    ok, err, idx = D.close_draws(bad, ref)
    off = int((np.abs(bad - ref) > D.GATE * max(1.0, np.abs(ref).max())).sum())
    print(f"draws-host | {kind} {size} {wrong}: {off} of {ref.size} elements off, largest {err:.3f} at {idx}")
    assert not ok and off >= 17, (wrong, off)


def test_the_gate_accepts_float32_and_rejects_one_element():
    ref = D.pose_noise(SEED, 0, 5, 3, 4, 3)
    ok, err, _ = D.close_draws(ref.astype(np.float32), ref)
    assert ok and 0 < err < 1e-6
    hit = ref.copy()
    hit[2, 2, 4, 1, 2, 16] += 1.1e-4 * max(1.0, np.abs(ref).max())
    assert D.close_draws(hit, ref)[::2] == (False, (2, 2, 4, 1, 2, 16))
    hit = ref.copy()
    hit[0, 0, 0, 0, 0, 0] = np.nan
    assert D.close_draws(hit, ref)[::2] == (False, (0,) * 6)


def _table_rows(text, macro):
    """the X(...) rows of `#define <macro>(X)` in the shipped-library half of mcd_instances.hpp -> lists of argument strings"""
    text = text[:text.index("// Developer builds")]
    body = re.search(r"#define " + macro + r"\(X\)((?:.*\\\n)*.*)\n", text).group(1)
    body = re.sub(r"/\*.*?\*/", "", body)
    return [[a.strip() for a in m.split(",")] for m in re.findall(r"X\(([^)]*)\)", body)]


def test_the_gpu_cases_cover_the_kernel_tables():
    """Every score_kernel row and every slab-tiled instance of csrc/mcd_instances.hpp has its in-kernel draw compared by
    tests/test_draws_gpu.py.  The lists restate the tables (non-LT rows) and are held against the header's text: a row added there
    is added here and then to the GPU module's cases."""
    import test_draws_gpu as G
    score_kernel = list(range(1, 13))                   # MCD_SCORE_INSTANCES: U-Net frames
    tiled = {16: (13, 16), 24: (17, 24), 32: (25, 32)}  # MCD_TILED_INSTANCES: padded size -> both ends of the frame counts it holds
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "mocodad_amd", "csrc", "mcd_instances.hpp")).read()
    assert sorted(int(r[1]) for r in _table_rows(src, "MCD_SCORE_INSTANCES") if r[4] == "false") == score_kernel
    assert sorted(int(r[1]) for r in _table_rows(src, "MCD_TILED_INSTANCES") if r[3] == "false") == sorted(tiled)
    assert sorted(int(r[1]) for r in _table_rows(src, "MCD_TILED_COND_INSTANCES")) == sorted(tiled)

    def frames(family, strategy):
        return {c["t_unet"] for c in G.CASES.values() if c["family"] == family and c["strategy"] == strategy}
    assert frames("score_kernel", "inject") == set(score_kernel)
    assert frames("score_kernel", "random_imp") == set(score_kernel) - {1}       # (a window of one frame has nothing to condition on)
    for name, c in G.CASES.items():
        if c["family"] == "score_kernel" and c["first"] == G.FIRST:
            assert c["splits"] == (0, 1, G.S), name
            assert c["fused"] == (c["t_unet"] in (3, 7, 12)), name
    for tp, ends in tiled.items():
        assert set(ends) <= frames("tiled", "concat"), tp
        assert tp in frames("tiled", "random_imp"), tp
    assert {17, 25} <= frames("tiled", "concat")
    assert {c["t_cond"] for c in G.CASES.values() if c["family"] == "tiled_cond"} == {13}       # the COND form, 16-frame instance
    assert {c["t_unet"] for c in G.CASES.values() if c["family"] == "generic"} == {1, 7, 12, 13, 32}
    lat = [c for c in G.CASES.values() if c["family"] == "latent"]
    assert {c["D"] for c in lat if c["t_unet"] == 3} == set(range(16, 129, 16))
    assert {(c["D"], c["t_unet"]) for c in lat if c["t_unet"] != 3} == {(32, 6), (32, 12)}
    for family in ("score_kernel", "tiled", "generic", "latent"):
        assert any(c["family"] == family and c["first"] == 2 ** 32 - 2 for c in G.CASES.values()), family
    assert G.EXPORT_POSE == [1, 2, 3, 7, 12, 13, 17, 32] and G.EXPORT_LATENT == list(range(16, 129, 16))
    assert G.FIRSTS == [0, 2 ** 32 - 2, -3, 2 ** 40 + 5] and (G.S, G.NS, G.B, G.SEED) == (3, 4, 5, SEED)
