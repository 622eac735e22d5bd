"""No GPU: the host side of mcd_latent_score_pose / mcd_latent_pose_workspace_bytes as far as it can be reached without a device.

No latent handle exists without a GPU (tests/test_latent_forecast_host.py), so what the call does with two handles -- the kinds, their
agreement, the alignment rules, the bits of every output -- is tests/test_latent_pose_call_gpu.py; this file holds the bindings, the
ABI version, the refusals that need no handle, and the module- and stream-level refusals that come before any device call."""
import ctypes as C

import pytest

from mocodad_amd import _lib

MCD_OK, MCD_EINVAL = 0, -1
P_ = C.c_void_p(0x1000)      # never dereferenced: a call that got past its checks would fault, a refused one returns


def _call(L, w, ae, cfg, data=P_, tab=P_, ws=P_, agg=P_, aggregation=_lib.AGGR["best"]):
    return L.mcd_latent_score_pose(w, ae, cfg, data, None, None, 0, 0, tab, ws, aggregation, C.c_float(0.0), agg, None, None, None, None,
                                   None, None)


def test_exports_are_bound_and_the_abi_version_stays():
    L = _lib.lib()
    for name in ("mcd_latent_score_pose", "mcd_latent_pose_workspace_bytes"):
        assert name in _lib.EXPORTS and hasattr(L, name)
    assert _lib.ABI_VERSION == 15 and L.mcd_abi_version() == 15          # two new exports, the version stays
    assert L.mcd_latent_score_pose.restype is C.c_int and len(L.mcd_latent_score_pose.argtypes) == 19
    assert L.mcd_latent_pose_workspace_bytes.restype is C.c_int64


def test_null_handles_and_null_workspace_are_einval():
    L = _lib.lib()
    err = lambda: L.mcd_last_error().decode()
    cfg = _lib.ScoreCfg()
    cfg.n_windows, cfg.n_samples, cfg.noise_steps, cfg.seg_len, cfg.n_cond, cfg.n_corrupt = 2, 2, 4, 6, 3, 3
    assert _call(L, None, None, None) == MCD_EINVAL and "null argument" in err()
    assert _call(L, None, None, C.byref(cfg)) == MCD_EINVAL and "null argument" in err() and "two handles" in err()
    assert _call(L, None, None, C.byref(cfg), ws=None) == MCD_EINVAL and "null argument" in err()
    assert _call(L, None, P_, C.byref(cfg)) == MCD_EINVAL and _call(L, P_, None, C.byref(cfg)) == MCD_EINVAL
    assert L.mcd_latent_pose_workspace_bytes(None, None, 5, 3) == 0


@pytest.mark.parametrize("n", [0, -3])
def test_no_windows_is_ok_before_anything_is_read(n):
    """n_windows <= 0: MCD_OK with every pointer NULL or bogus -- nothing is dereferenced, no device call is made (there is no
    device here)."""
    L = _lib.lib()
    cfg = _lib.ScoreCfg()
    cfg.n_windows = n
    assert _call(L, None, None, C.byref(cfg), data=None, tab=None, ws=None, agg=None) == MCD_OK
    assert _call(L, P_, P_, C.byref(cfg)) == MCD_OK
    assert L.mcd_latent_pose_workspace_bytes(P_, P_, n, 3) == 0


# ---------------------------------------------------------------- the module and the stream, before any device call
@pytest.fixture()
def model_and_stage1():
    from test_latent_forecast_host import _models
    m, sd = _models()
    yield m, sd
    m._decoder_sd = m._decoder = m._pose_scorer = None


def test_pose_scorer_needs_a_decoder_and_a_device(model_and_stage1):
    """Without a decoder (and, for a module on the CPU, without a cuda device: the session shares this module, which a GPU test may
    have moved) pose_scorer() raises before a decoder is packed."""
    m, _ = model_and_stage1
    assert m._decoder_sd is None
    with pytest.raises(RuntimeError, match="cuda device|load_decoder"):
        m.pose_scorer()
    assert m._decoder is None


def test_engine_class_refuses_other_objects():
    from mocodad_amd.engine import LatentPoseScorer
    with pytest.raises(TypeError, match="LatentScorer"):
        LatentPoseScorer(object(), object())


class _FakeLatent:
    is_latent = True


def test_stream_refusals_of_a_latent_module_in_latent_space_are_unchanged():
    from mocodad_amd.stream import ForecastCfg, PoseStream
    with pytest.raises(NotImplementedError, match="a latent has no joints"):
        PoseStream(_FakeLatent(), vid_res=(640, 360), joint_scores=True)
    with pytest.raises(NotImplementedError, match="needs the pose model"):
        PoseStream(_FakeLatent(), vid_res=(640, 360), forecasts=ForecastCfg())
    with pytest.raises(NotImplementedError, match="a latent has no joints"):
        PoseStream(_FakeLatent(), vid_res=(640, 360), joint_scores=True, space="latent")
    with pytest.raises(ValueError, match="space must be"):
        PoseStream(_FakeLatent(), vid_res=(640, 360), space="joint")


def test_stream_space_is_for_the_latent_model():
    from mocodad_amd.stream import PoseStream

    class Pose:
        pass
    with pytest.raises(ValueError, match="space= is for the latent model"):
        PoseStream(Pose(), vid_res=(640, 360), space="pose")
