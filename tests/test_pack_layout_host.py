"""CPU: the packed weight layout, pinned without a GPU.  mcd_debug_pack_digest runs the host packer (mocodad_amd/csrc/mcd_pack.hpp) and
returns the buffer's float count and an FNV-1a digest over the buffer and the tables the handle keeps; tests/golden/pack_digests.json
holds both for every case below, recorded from the commit named in the file (its packer, before mcd_pack.hpp existed, patched in a
scratch copy with the same export; the file's "how" entry says what was hashed and how that commit's CondW, whose per-layer arrays
have since become GLayer rows, was laid out for it, so that the digests can be recorded again from that commit).  A byte of the
buffer or a table word that moves fails here.

The weights of a case come from numpy.random.default_rng(case index), not from torch's generator: the values do not depend on
the torch version.  The error cases assert code and mcd_last_error() text literally, as that commit's library reported them."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import latent_ref
from conftest import GOLDEN
from helpers import golden_weights, make_args
from mocodad_amd import _lib
from mocodad_amd.engine import _pack_tensors
from mocodad_amd.models.mocodad import MoCoDAD
from mocodad_amd.models.mocodad_latent import MoCoDADlatent

SHIPPED = dict(conditioning_architecture="AE", channels=[32, 16, 32], h_dim=32)      # + h_dim: the channel list 32, 16, 32, 32
OTHER = dict(conditioning_architecture="E", channels=[24, 40], h_dim=8)              # three layers, none of the shipped widths


def _concat(T):
    return dict(conditioning_strategy="concat", seg_len=T, conditioning_indices=[0])


def _inject(t_cond, **enc):
    return dict(conditioning_strategy="inject", seg_len=t_cond + 3, conditioning_indices=list(range(t_cond)), **enc)


# (name, latent model?, settings over the golden configuration).  Each packer branch has a case:
CASES = [
    # U-Net frame counts of the specialised kernels ...
    ("unet3", False, _concat(3)), ("unet6", False, _concat(6)), ("unet7", False, _concat(7)), ("unet12", False, _concat(12)),
    # ... and of the tiled tables (13 pads to 16)
    ("unet13", False, _concat(13)), ("unet16", False, _concat(16)), ("unet24", False, _concat(24)), ("unet32", False, _concat(32)),
    ("no_condition", False, dict(conditioning_strategy="no_condition", seg_len=6)),
    # 'inject', shipped channel list: the fast table (3, 12 condition frames); plain rows only (24); plain rows whose third
    # activation buffer no longer fits LDS (28: CondW::gmode)
    ("inject_c3", False, _inject(3, **SHIPPED)), ("inject_c12", False, _inject(12, **SHIPPED)),
    ("inject_c24", False, _inject(24, **SHIPPED)), ("inject_c28", False, _inject(28, **SHIPPED)),
    ("inject_other_list", False, _inject(3, **OTHER)),
    ("eunet_c3", False, _inject(3, conditioning_architecture="E_unet")),
    ("eunet_c16", False, _inject(16, conditioning_architecture="E_unet")),          # tiled condition tables
    # latent model: shipped encoder at 3 + 3 (fused table) with a 2-layer denoiser; 5 condition frames (fast, not fused);
    # 'E_unet'; another channel list; a 5-layer denoiser of other widths
    ("latent_ae_3_3", True, dict(_inject(3, **SHIPPED), latent_embedding_dim=32, hidden_sizes=[48, 32])),
    ("latent_ae_5_3", True, dict(_inject(5, **SHIPPED), latent_embedding_dim=32, hidden_sizes=[48, 32])),
    ("latent_eunet", True, dict(_inject(3, conditioning_architecture="E_unet"), latent_embedding_dim=64, hidden_sizes=[64, 128, 128, 64])),
    ("latent_other_list", True, dict(_inject(3, **OTHER), latent_embedding_dim=16, hidden_sizes=[16])),
    ("latent_5_layers", True, dict(_inject(3, **SHIPPED), latent_embedding_dim=80, hidden_sizes=[96, 32, 128, 16, 80])),
]
IDS = [c[0] for c in CASES]


def build_inputs(index):
    """-> (state_dict with every floating tensor drawn from default_rng(index), ModelCfg, LatentCfg | None)"""
    _, latent, over = CASES[index]
    base = latent_ref.load_fixture("B")[2] if latent else golden_weights("inject")[1]
    with torch.no_grad():
        m = (MoCoDADlatent if latent else MoCoDAD)(make_args(base, **over))
    rng = np.random.default_rng(index)
    sd = {}
    for k, v in m.state_dict().items():
        if not v.dtype.is_floating_point:
            continue
        a = rng.standard_normal(tuple(v.shape))
        if k.endswith("running_var"):
            a = np.abs(a) + 0.5
        sd[k] = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32).reshape(tuple(v.shape)))
    ci, xi = m._frame_split()
    s = m.conditioning_strategy
    unet_enc = m.conditioning_architecture == "E_unet"
    chans = list(m.condition_encoder.channels) if m.condition_encoder is not None and not unet_enc else []
    cfg = _lib.ModelCfg(num_coords=2, n_joints=17, emb_dim=16, strategy=_lib.STRATEGY[s])
    cfg.t_cond = len(ci) if s == "inject" else 0
    cfg.t_unet = len(xi) + (len(ci) if s in ("concat", "inbetween_imp", "random_imp") else 0)
    cfg.cond_layers = _lib.COND_UNET if unet_enc else len(chans)
    for i, c in enumerate(chans):
        cfg.cond_channels[i] = c
    lcfg = None
    if latent:
        lcfg = _lib.LatentCfg(latent_dim=m.latent_embedding_dim, n_layers=len(m.hidden_sizes))
        for i, h in enumerate(m.hidden_sizes):
            lcfg.hidden[i] = h
    return sd, cfg, lcfg


def pack_digest(L, sd, cfg, lcfg):
    """-> (return code, n_floats, digest) of mcd_debug_pack_digest"""
    arr, n, keep = _pack_tensors(sd)
    nf, dg = C.c_int64(0), C.c_uint64(0)
    rc = L.mcd_debug_pack_digest(arr, n, C.byref(cfg), C.byref(lcfg) if lcfg is not None else None, C.byref(nf), C.byref(dg))
    del keep
    return rc, int(nf.value), int(dg.value)


def recorded():
    with open(os.path.join(GOLDEN, "pack_digests.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("index", range(len(CASES)), ids=IDS)
def test_packed_layout_matches_the_recorded_digest(index):
    L = _lib.lib()
    rc, n_floats, digest = pack_digest(L, *build_inputs(index))
    assert rc == 0, L.mcd_last_error()
    want = recorded()["cases"][CASES[index][0]]
    print(f"{CASES[index][0]}: n_floats {n_floats} digest {digest:016x}  recorded {want['n_floats']} {want['digest']}")
    assert n_floats == want["n_floats"]
    assert f"{digest:016x}" == want["digest"]


def test_case_list_holds_the_configurations_it_names():
    """The configurations behind the case names: frame counts, channel lists, layer counts, and that 28 condition frames (not 24)
    are where three activation buffers outgrow LDS.  Which tables the packer writes for them is not visible from here: the digest
    covers that (gmode, the fast table's words and tiled_tp are part of what it hashes)."""
    def cfg_of(name):
        return build_inputs(IDS.index(name))[1]
    assert [cfg_of(f"unet{t}").t_unet for t in (3, 6, 7, 12, 13, 16, 24, 32)] == [3, 6, 7, 12, 13, 16, 24, 32]
    assert cfg_of("inject_c12").t_cond == 12 and list(cfg_of("inject_c12").cond_channels)[:4] == [32, 16, 32, 32]
    assert cfg_of("inject_c24").t_cond == 24 and cfg_of("inject_c28").t_cond == 28
    # three activation buffers of the shipped list (32 channels x T_c x 17 floats, + 512 partial sums) against 160 KB of LDS
    assert (3 * 32 * 24 * 17 + 512) * 4 <= 160 * 1024 < (3 * 32 * 28 * 17 + 512) * 4
    assert cfg_of("inject_other_list").cond_layers == 3
    assert cfg_of("eunet_c16").cond_layers == _lib.COND_UNET and cfg_of("eunet_c16").t_cond == 16
    assert cfg_of("no_condition").cond_layers == 0 and cfg_of("unet6").cond_layers == 0
    assert build_inputs(IDS.index("latent_5_layers"))[2].n_layers == 5 and build_inputs(IDS.index("latent_ae_3_3"))[2].n_layers == 2
    assert set(recorded()["cases"]) == set(IDS)


# The autoencoder of stage 'pretrain' (pack_latent_ae_model, behind mcd_debug_pack_ae_digest): (name, corrupt frames, settings).
# The shipped encoder at 3 + 3 (fused table); 5 corrupt + 3 condition frames (fast, not fused; to_time_dim as fragments); 'E_unet' at
# 12 + 12; another channel list at 6 + 3.  Their digests ("ae_cases" of pack_digests.json, "ae_recorded_from") were recorded the same
# way from the commit that added the stage, patched with this export alone.
AE_CASES = [
    ("ae_3_3", 3, dict(_inject(3, **SHIPPED), latent_embedding_dim=32)),
    ("ae_5_3", 5, dict(_inject(3, **SHIPPED), latent_embedding_dim=32)),
    ("ae_eunet_12_12", 12, dict(_inject(12, conditioning_architecture="E_unet"), latent_embedding_dim=64)),
    ("ae_other_list_6_3", 6, dict(_inject(3, **OTHER), latent_embedding_dim=16)),
]
AE_IDS = [c[0] for c in AE_CASES]


def build_ae_inputs(index):
    """-> (state_dict drawn from default_rng(1000 + index), ModelCfg, latent_dim) of AE_CASES[index]"""
    import latentp_ref
    from mocodad_amd.models.mocodad_latent_pretrain import MoCoDADlatentPretrain
    _, t_corrupt, over = AE_CASES[index]
    t_cond = len(over["conditioning_indices"])
    base = dict(latentp_ref.load_fixture("P6")[2], stage="pretrain")
    with torch.no_grad():
        m = MoCoDADlatentPretrain(make_args(base, **dict(over, seg_len=t_cond + t_corrupt)))
    rng = np.random.default_rng(1000 + index)
    sd = {}
    for k, v in m.state_dict().items():
        if not v.dtype.is_floating_point:
            continue
        a = rng.standard_normal(tuple(v.shape))
        if k.endswith("running_var"):
            a = np.abs(a) + 0.5
        sd[k] = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32).reshape(tuple(v.shape)))
    ci, xi = m._frame_split()
    unet_enc = m.conditioning_architecture == "E_unet"
    chans = [] if unet_enc else list(m.condition_encoder.channels)
    cfg = _lib.ModelCfg(num_coords=2, n_joints=17, emb_dim=16, strategy=_lib.STRATEGY["inject"])
    cfg.t_cond, cfg.t_unet = len(ci), len(xi)
    cfg.cond_layers = _lib.COND_UNET if unet_enc else len(chans)
    for i, c in enumerate(chans):
        cfg.cond_channels[i] = c
    return sd, cfg, m.latent_embedding_dim


@pytest.mark.parametrize("index", range(len(AE_CASES)), ids=AE_IDS)
def test_autoencoder_packed_layout_matches_the_recorded_digest(index):
    L = _lib.lib()
    sd, cfg, D = build_ae_inputs(index)
    name, t_corrupt, over = AE_CASES[index]
    assert (cfg.t_unet, cfg.t_cond, D) == (t_corrupt, len(over["conditioning_indices"]), over["latent_embedding_dim"])
    arr, n, keep = _pack_tensors(sd)
    nf, dg = C.c_int64(0), C.c_uint64(0)
    rc = L.mcd_debug_pack_ae_digest(arr, n, C.byref(cfg), D, C.byref(nf), C.byref(dg))
    del keep
    assert rc == 0, L.mcd_last_error()
    want = recorded()["ae_cases"][name]
    print(f"{name}: n_floats {nf.value} digest {dg.value:016x}  recorded {want['n_floats']} {want['digest']}")
    assert int(nf.value) == want["n_floats"]
    assert f"{dg.value:016x}" == want["digest"]
    assert set(recorded()["ae_cases"]) == set(AE_IDS)


def _without(sd, key):
    assert key in sd
    return {k: v for k, v in sd.items() if k != key}


# (case, tensor to drop or resize, code, mcd_last_error() text): one missing tensor in each encoder branch -- 'E_unet', plain rows,
# and the plain branch of a handle that also packs the fast table -- and a wrong element count
ERRORS = [
    ("eunet_c3", "drop", "condition_encoder.st_gcnnsd2.0.residual.1.running_mean", -2,
     "missing tensor condition_encoder.st_gcnnsd2.0.residual.1.running_mean"),
    ("eunet_c16", "drop", "condition_encoder.down2.block.0.bias", -2, "missing tensor condition_encoder.down2.block.0.bias"),
    ("inject_other_list", "drop", "condition_encoder.encoder.model_layers.1.prelu.weight", -2,
     "missing tensor condition_encoder.encoder.model_layers.1.prelu.weight"),
    ("inject_c3", "drop", "condition_encoder.encoder.model_layers.2.gcn.A", -2,
     "missing tensor condition_encoder.encoder.model_layers.2.gcn.A"),
    ("inject_c3", "drop", "condition_encoder.btlnk.bias", -2, "missing tensor condition_encoder.btlnk.bias"),
    ("latent_ae_3_3", "drop", "condition_encoder.encoder.model_layers.3.tcn.0.weight", -2,
     "missing tensor condition_encoder.encoder.model_layers.3.tcn.0.weight"),
    ("unet13", "drop", "model.up3.block.1.weight", -2, "missing tensor model.up3.block.1.weight"),
    ("latent_5_layers", "drop", "denoiser.net.3.1.running_var", -2, "missing tensor denoiser.net.3.1.running_var"),
    ("inject_c3", "grow", "condition_encoder.encoder.model_layers.0.tcn.0.weight", -2,
     "tensor condition_encoder.encoder.model_layers.0.tcn.0.weight has 65 elements, expected 64"),
    ("unet6", "grow", "model.st_gcnnsd3.1.gcn.T", -2, "tensor model.st_gcnnsd3.1.gcn.T has 361 elements, expected 360"),
]


@pytest.mark.parametrize("case,how,key,code,text", ERRORS, ids=[f"{e[0]}-{e[1]}-{i}" for i, e in enumerate(ERRORS)])
def test_packer_errors_are_reported_as_before(case, how, key, code, text):
    L = _lib.lib()
    sd, cfg, lcfg = build_inputs(IDS.index(case))
    if how == "drop":
        sd = _without(sd, key)
    else:
        sd = dict(sd)
        sd[key] = torch.cat([sd[key].reshape(-1), torch.zeros(1)])
    rc, _, _ = pack_digest(L, sd, cfg, lcfg)
    print(f"{case} {how} {key}: rc {rc} '{L.mcd_last_error().decode()}'")
    assert rc == code
    assert L.mcd_last_error().decode() == text
    # the packers proper report the same (they fail before their first device call)
    arr, n, keep = _pack_tensors(sd)
    h = C.c_void_p()
    if lcfg is None:
        rc2 = L.mcd_pack_weights(arr, n, C.byref(cfg), 0, C.byref(h))
    else:
        rc2 = L.mcd_pack_latent_weights(arr, n, C.byref(cfg), C.byref(lcfg), 0, C.byref(h))
    assert rc2 == code and L.mcd_last_error().decode() == text
