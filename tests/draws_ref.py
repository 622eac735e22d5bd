"""NumPy restatement of the noise draws of a chain (include/mocodad_hip.h: mcd_philox_noise, mcd_latent_philox_noise), written
from the key layout alone.  Test code only: nothing under mocodad_amd/ imports it.  tests/test_draws_host.py checks the
restatement and the sharpness of the gate on the CPU; tests/test_draws_gpu.py holds the exported tensors, and through them the
in-kernel draws of every trajectory kernel row, against it.

KEY LAYOUT.  A Philox4x32-10 call (rndimp_ref.philox4x32_10) has the key (low, high 32 bits of `seed`) and the counter
(c0, c1, c2, c3):
  c1 = noise slot k: 0 = x_T, k >= 1 = the z of step ns - k          c2 = sample s
  c3 = (first_window_id + b) mod 2^32, the global id of window b of the call
  c0 = pose x_T:      (c * Tx + tx) * 17 + v: one call per element (coordinate c, corrupt frame tx of Tx, joint v);
                      z = r(w0) cos(a(w1)), words w2 and w3 unused
       pose step k:   tx * 9 + v0 / 2: one call per joint pair (v0 even) of frame tx.  (w0, w1) give coordinates 0, 1 of joint v0
                      as (r cos, r sin), (w2, w3) the same of joint v0 + 1 (unused at v0 = 16)
       latent, any k: d0 / 4: one call per group of four elements d0 .. d0 + 3, in the order r(w0) cos(a(w1)), r(w0) sin(a(w1)),
                      r(w2) cos(a(w3)), r(w2) sin(a(w3))
Box-Muller: u(w) = (float32(w >> 8) + 0.5f) * 2^-24 evaluated in float32 (every step is exactly reproducible; the largest word
rounds to u = 1 and gives r = 0); r(w) = sqrt(float32(-1.38629436111989) * log2(u(w))), a(w) = float32(6.28318530717958647692)
* u(w), both evaluated in float64 from the float32 u (the kernels use the hardware log2, sqrt, sin and cos).
Layouts: poses (S, K, B, 2, Tx, 17), latents (S, K, B, D), K = max(ns - 1, 1), slot k at index k.

`wrong` names ONE deliberate single-field mistake (MISTAKES): the host test proves that the gate of the GPU test, close_draws,
rejects each of them, so a kernel that made it could not pass.
"""
import numpy as np

from rndimp_ref import M32, philox4x32_10

GATE = 1e-4             # the project's hard gate: |got - ref64| <= GATE * max(1, max|ref64|), per element
# single-field mistakes of a draw: name -> which restatement it applies to
MISTAKES = {
    "c1_c2_swapped": ("pose", "latent"),        # slot and sample exchanged in the counter
    "slot_k-1": ("pose", "latent"),             # slot k - 1 for k
    "sample_0": ("pose", "latent"),             # sample 0 for every s
    "window_no_wrap": ("pose", "latent"),       # the window id saturates at 2^32 - 1 instead of wrapping
    "xT_Tx+1": ("pose",),                       # Tx + 1 in the x_T element index
    "step_tx*8": ("pose",),                     # tx * 8 for tx * 9 in the joint-pair index
    "cos_sin_swapped": ("pose", "latent"),
    "w1_w2_swapped": ("pose", "latent"),        # output words 1 and 2 exchanged
    "latent_d0/8": ("latent",),                 # the element group d0 / 8 for d0 / 4
    "seed_high_ignored": ("pose", "latent"),    # key word 1 = 0
}
_F32_R = np.float64(np.float32(-1.38629436111989))
_F32_2PI = np.float64(np.float32(6.28318530717958647692))


def n_slots(ns: int) -> int:
    return max(int(ns) - 1, 1)


def window_ids(first, B, wrong=None):
    """(B,) uint64: (first + b) mod 2^32 -- from Python integers, so a negative or a 40-bit `first` wraps like the int64 does"""
    if wrong == "window_no_wrap":
        return np.array([min((int(first) & (2 ** 64 - 1)) + b, 0xFFFFFFFF) for b in range(B)], dtype=np.uint64)
    return np.array([(int(first) + b) & 0xFFFFFFFF for b in range(B)], dtype=np.uint64)


def uniform(w):
    """float32 u of a 32-bit word: every operation in float32, as the kernels evaluate it"""
    return ((np.asarray(w, dtype=np.uint64) >> np.uint64(8)).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -24)


def box_muller(wa, wb, wrong=None):
    """words -> (r cos a, r sin a) in float64 from the float32 uniforms"""
    u1, u2 = uniform(wa), uniform(wb)
    assert u1.dtype == np.float32 and u2.dtype == np.float32
    r = np.sqrt(_F32_R * np.log2(u1.astype(np.float64))) + 0.0          # (u = 1: sqrt(-0.0) + 0.0 = 0.0)
    a = _F32_2PI * u2.astype(np.float64)
    return (r * np.sin(a), r * np.cos(a)) if wrong == "cos_sin_swapped" else (r * np.cos(a), r * np.sin(a))


def _call(seed, c0, k, s, win, wrong=None):
    """One Philox call per broadcast element of (c0, k, s, win) -> ((c0, c1, c2, c3) as sent, (w0, w1, w2, w3))"""
    k, s = np.asarray(k, dtype=np.int64), np.asarray(s, dtype=np.int64)
    if wrong == "slot_k-1":
        k = k - 1
    if wrong == "sample_0":
        s = np.zeros_like(s)
    c1, c2 = (s, k) if wrong == "c1_c2_swapped" else (k, s)
    if wrong == "seed_high_ignored":
        seed = int(seed) & 0xFFFFFFFF
    ctr = tuple(np.asarray(c).astype(np.uint64) & M32 for c in np.broadcast_arrays(np.asarray(c0, dtype=np.int64), c1, c2, win.astype(np.int64)))
    w = philox4x32_10(seed, *ctr)
    if wrong == "w1_w2_swapped":
        w = (w[0], w[2], w[1], w[3])
    return ctr, w


def pose_calls(seed, first, B, S, ns, Tx, wrong=None):
    """-> [x_T calls, step calls]: each (counter words, output words), shaped (S, B, 2, Tx, 17) and (S, K - 1, B, Tx, 9)"""
    K, win = n_slots(ns), window_ids(first, B, wrong)
    s, c, tx, v = np.arange(S), np.arange(2), np.arange(Tx), np.arange(17)
    tx_e = Tx + 1 if wrong == "xT_Tx+1" else Tx
    e = (c[:, None, None] * tx_e + tx[None, :, None]) * 17 + v[None, None, :]
    xt = _call(seed, e[None, None], 0, s[:, None, None, None, None], win[None, :, None, None, None], wrong)
    k, jp = np.arange(1, K), np.arange(9)
    pair = tx[:, None] * (8 if wrong == "step_tx*8" else 9) + jp[None, :]
    step = _call(seed, pair[None, None, None], k[None, :, None, None, None], s[:, None, None, None, None],
                 win[None, None, :, None, None], wrong)
    return [xt, step]


def _pose_layout(pair, seed, first, B, S, ns, Tx, wrong=None):
    """pair(wa, wb) -> the two values a word pair gives, laid out as (S, K, B, 2, Tx, 17)"""
    K = n_slots(ns)
    (_, wx), (_, ws) = pose_calls(seed, first, B, S, ns, Tx, wrong)
    out = np.full((S, K, B, 2, Tx, 17), np.nan)
    out[:, 0] = pair(wx[0], wx[1])[0]
    if K > 1:
        a0, a1 = pair(ws[0], ws[1])          # joint v0:     coordinates 0, 1
        b0, b1 = pair(ws[2], ws[3])          # joint v0 + 1: coordinates 0, 1 (the ninth pair has none)
        out[:, 1:, :, 0, :, 0::2], out[:, 1:, :, 1, :, 0::2] = a0, a1
        out[:, 1:, :, 0, :, 1::2], out[:, 1:, :, 1, :, 1::2] = b0[..., :8], b1[..., :8]
    return out


def pose_noise(seed, first, B, S, ns, Tx, wrong=None):
    """-> (S, K, B, 2, Tx, 17) float64: the tensor mcd_philox_noise(seed, first, B, S, ns, Tx) exports"""
    return _pose_layout(lambda wa, wb: box_muller(wa, wb, wrong), seed, first, B, S, ns, Tx, wrong)


def pose_uniforms(seed, first, B, S, ns, Tx):
    """-> (u1, u2), each in the layout of pose_noise: the uniforms every element is computed from"""
    return (_pose_layout(lambda wa, wb: (uniform(wa),) * 2, seed, first, B, S, ns, Tx),
            _pose_layout(lambda wa, wb: (uniform(wb),) * 2, seed, first, B, S, ns, Tx))


def latent_calls(seed, first, B, S, ns, D, wrong=None):
    """-> [(counter words, output words)] shaped (S, K, B, D / 4)"""
    assert D % 4 == 0
    K, win = n_slots(ns), window_ids(first, B, wrong)
    d0 = 4 * np.arange(D // 4)
    grp = d0 // (8 if wrong == "latent_d0/8" else 4)
    return [_call(seed, grp[None, None, None], np.arange(K)[None, :, None, None], np.arange(S)[:, None, None, None],
                  win[None, None, :, None], wrong)]


def _latent_layout(pair, seed, first, B, S, ns, D, wrong=None):
    (_, w), = latent_calls(seed, first, B, S, ns, D, wrong)
    a0, a1 = pair(w[0], w[1])
    b0, b1 = pair(w[2], w[3])
    return np.stack([a0, a1, b0, b1], axis=-1).reshape(S, n_slots(ns), B, D).astype(np.float64)


def latent_noise(seed, first, B, S, ns, D, wrong=None):
    """-> (S, K, B, D) float64: the tensor mcd_latent_philox_noise(seed, first, B, S, ns, D) exports"""
    return _latent_layout(lambda wa, wb: box_muller(wa, wb, wrong), seed, first, B, S, ns, D, wrong)


def latent_uniforms(seed, first, B, S, ns, D):
    """-> (u1, u2), each in the layout of latent_noise"""
    return (_latent_layout(lambda wa, wb: (uniform(wa),) * 2, seed, first, B, S, ns, D),
            _latent_layout(lambda wa, wb: (uniform(wb),) * 2, seed, first, B, S, ns, D))


def close_draws(a, ref):
    """The gate of tests/test_draws_gpu.py on an exported tensor: every element finite and within GATE * max(1, max|ref|) of the
    float64 restatement.  -> (passes, largest |a - ref|, index of that element)"""
    a, ref = np.asarray(a, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert a.shape == ref.shape and ref.dtype == np.float64 and np.isfinite(ref).all(), (a.shape, ref.shape)
    d = np.abs(a - ref)
    d[~np.isfinite(d)] = np.inf
    idx = np.unravel_index(int(np.argmax(d)), d.shape)
    err = float(d[idx])
    return bool(err <= GATE * max(1.0, float(np.abs(ref).max()))), err, tuple(int(i) for i in idx)
