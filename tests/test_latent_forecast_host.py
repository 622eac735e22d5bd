"""No GPU: the host side of "decode generated latents to poses" -- the two exports of mcd_latent_decode_samples as far as they can
be reached without a device, and MoCoDADlatent.load_decoder / latent_score_space.

No latent handle exists without a GPU (a packer call that passes every check ends in MCD_EDEVICE here: tests/test_latentp_golden.py),
so what the library does with a handle -- the diffusion-stage handle's MCD_EUNSUPPORTED, n_samples = 0, misaligned latents, NULL
outputs, the workspace query's monotony and bound -- is tests/test_latent_forecast_gpu.py::test_rejected_calls and
::test_workspace_query; this file holds the refusals that need none."""
import ctypes as C

import pytest
import torch

import latent_ref as LR
from helpers import make_args
from mocodad_amd import _lib

MCD_EINVAL = -1


def test_exports_and_calls_without_a_handle():
    L = _lib.lib()
    for name in ("mcd_latent_decode_samples", "mcd_latent_decode_workspace_bytes"):
        assert name in _lib.EXPORTS and hasattr(L, name)
    assert _lib.ABI_VERSION == 15 and L.mcd_abi_version() == 15          # two new exports, the version stays
    assert _lib.LATENT_OPT == {"split_encode": 0, "decode_spw": 1, "decode_chunk": 2}
    assert L.mcd_latent_decode_samples(None, None, None, None, None, None, None, None, None, None, None) == MCD_EINVAL
    assert "null argument" in L.mcd_last_error().decode()
    cfg = _lib.ScoreCfg()
    assert L.mcd_latent_decode_samples(None, C.byref(cfg), None, None, None, None, None, None, None, None, None) == MCD_EINVAL
    assert L.mcd_latent_decode_workspace_bytes(None, 5, 3) == 0
    assert L.mcd_latent_set_option(None, _lib.LATENT_OPT["decode_spw"], 1) == MCD_EINVAL


# ---------------------------------------------------------------- the module
def _models(D=32):
    """-> (MoCoDADlatent, stage-1 state_dict whose shared tensors are the module's): fixture B's 3 + 3 frame settings"""
    from mocodad_amd.models.mocodad_latent_pretrain import MoCoDADlatentPretrain
    m, _ = LR.random_latent_model(D, [48, D], seed=31, ns=4, S=3, tame=True)
    cfg = LR.load_fixture("B")[2]
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(32)
        sd = {k: v.detach().clone() for k, v in MoCoDADlatentPretrain(make_args(cfg, stage="pretrain", latent_embedding_dim=D)).state_dict().items()}
    own = m.state_dict()
    assert all(k in sd for k in own if k.startswith(("model.", "condition_encoder.")))
    sd.update({k: v.detach().clone() for k, v in own.items() if k in sd})
    return m, sd


@pytest.fixture()
def model_and_stage1():
    m, sd = _models()
    yield m, sd
    m._decoder_sd = m._decoder = None      # (the module is shared by the session: leave it as it was)


def test_load_decoder_checks_the_shared_tensors(model_and_stage1):
    m, sd = model_and_stage1
    keys = list(m.state_dict())
    shared = [k for k in keys if k.startswith(("model.", "condition_encoder.")) and m.state_dict()[k].dtype.is_floating_point]
    for k in (shared[0], [k for k in shared if "to_time_dim" in k][0], [k for k in shared if k.startswith("condition_encoder.")][-1]):
        bad = dict(sd)
        bad[k] = sd[k] + 1
        with pytest.raises(ValueError) as e:
            m.load_decoder(bad)
        assert repr(k) in str(e.value) and m._decoder_sd is None, (k, str(e.value))
        m.load_decoder(bad, check=False)                   # accepted: the module's own tensor decodes
        assert torch.equal(m._decoder_sd[k], m.state_dict()[k].cpu())
        m._decoder_sd = None
    # the FIRST differing key, in the module's own key order
    bad = dict(sd)
    bad[shared[5]], bad[shared[2]] = sd[shared[5]] + 1, sd[shared[2]] + 1
    with pytest.raises(ValueError, match=repr(shared[2]).replace(".", r"\.")):
        m.load_decoder(bad)
    with pytest.raises(ValueError, match="rev_to_time_dim"):
        m.load_decoder({k: v for k, v in sd.items() if "rev_to_time_dim" not in k})
    m.load_decoder(sd)
    assert list(m.state_dict()) == keys                    # nothing registered
    assert not any("decoder" in n for n, _ in m.named_parameters() if n.startswith("_"))
    assert {k.split(".")[1] for k in m._decoder_sd if k.startswith("model.")} >= {"rev_to_time_dim", "up3", "up2", "st_gcnnsu4", "st_gcnnsu3"}
    assert not any(k.startswith("denoiser.") for k in m._decoder_sd)
    m.load_state_dict(m.state_dict())                      # a diffusion checkpoint loads as before, and drops the decoder
    assert m._decoder_sd is None


def test_load_decoder_sources(model_and_stage1, tmp_path):
    m, sd = model_and_stage1
    path = tmp_path / "stage1.ckpt"
    torch.save({"state_dict": sd}, path)
    m.load_decoder(str(path))
    assert m._decoder_sd is not None
    m._decoder_sd = None
    old = m.pretrained_model_ckpt_path
    try:
        m.pretrained_model_ckpt_path = str(path)           # None = the reference's own key
        m.load_decoder()
        assert m._decoder_sd is not None
        m.pretrained_model_ckpt_path = str(tmp_path / "missing.ckpt")
        with pytest.raises(FileNotFoundError):
            m.load_decoder()
        m.pretrained_model_ckpt_path = None
        with pytest.raises(ValueError, match="pretrained_model_ckpt_path"):
            m.load_decoder()
    finally:
        m.pretrained_model_ckpt_path = old


def test_refusals_without_a_decoder(model_and_stage1):
    m, _ = model_and_stage1
    assert m.latent_score_space == "latent"
    with pytest.raises(RuntimeError, match="load_decoder"):
        m.forward([None, None, None, None], space="pose")                  # before the inputs are touched
    with pytest.raises(NotImplementedError, match="a latent has no joints") as e:
        m.forward([None, None, None, None], return_maps=True)
    assert "load_decoder" in str(e.value)
    with pytest.raises(RuntimeError, match="load_decoder"):
        m.decoder()


def test_unknown_score_space(model_and_stage1):
    from mocodad_amd.models.mocodad_latent import MoCoDADlatent
    m, _ = model_and_stage1
    with pytest.raises(ValueError, match="latent_score_space"):
        m.forward([None, None, None, None], space="joint")
    cfg = LR.load_fixture("B")[2]
    with pytest.raises(ValueError, match="latent_score_space"):
        MoCoDADlatent(make_args(cfg, latent_score_space="joint"))
    assert MoCoDADlatent(make_args(cfg, latent_score_space="pose")).latent_score_space == "pose"


def test_the_new_config_loads():
    import os
    from mocodad_amd.utils.argparser import load_config
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    a = load_config(os.path.join(root, "configs", "ubnormal_latent_pose_test.yaml"))
    b = load_config(os.path.join(root, "configs", "ubnormal_latent_test.yaml"))
    assert a.latent_score_space == "pose" and not hasattr(b, "latent_score_space")
    assert {k: v for k, v in vars(a).items() if k != "latent_score_space"} == vars(b)
