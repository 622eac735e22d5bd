"""GPU: calls on a packed handle that host validation rejects -- none reaches a launch; each must keep its return code and its
mcd_last_error() text.  The expected pairs are tests/golden/call_errors.json["gpu"], recorded on the MI355X from the library
before the call front end (mcd_call.hpp) existed:

    python tests/test_call_errors_gpu.py --record      # rewrites the "gpu" key; see the file's "how" entry

The calls go through ctypes with real device buffers of the call's sizes (3 windows, 2 samples, 4 steps)."""
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_call_errors_host import JSON, NAN, expected, record, run_case, view  # noqa: E402

from mocodad_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu
B, S, NS = 3, 2, 4
_ctx = {}


def _ptr(t, off=0):
    return None if t is None else C.c_void_p(t.data_ptr() + off)


def make_cfg(p, **over):
    """The ScoreCfg of a (B, S, NS) call on p's handle, with fields or single list entries replaced."""
    sc = p.sc
    c = _lib.ScoreCfg()
    c.n_windows, c.n_samples, c.noise_steps, c.seg_len = over.pop("B", B), over.pop("S", S), over.pop("ns", NS), sc.seg_len
    c.n_cond, c.n_corrupt, c.loss_fn = len(sc.cond_idx), len(sc.corrupt_idx), 0
    for i, v in enumerate(sc.cond_idx):
        c.cond_idx[i] = v
    for i, v in enumerate(sc.corrupt_idx):
        c.corrupt_idx[i] = v
    for k, v in over.items():
        if k in ("cond_idx", "corrupt_idx"):
            for i, x in v.items():
                getattr(c, k)[i] = x
        else:
            setattr(c, k, v)
    return c


class Pose:
    """A pose handle and the buffers of one (B, S, NS) call."""

    def __init__(self, variant):
        from oracle import mocodad_oracle as O
        from helpers import golden_weights
        from mocodad_amd.engine import HipScorer
        sd, cfg = golden_weights(variant)
        strat = cfg["conditioning_strategy"]
        if strat == "random_imp":
            k = cfg["conditioning_indices"]
            ci, xi = list(range(k)), list(range(k, cfg["seg_len"]))
        else:
            ci, xi = O.split_indices(cfg["seg_len"], cfg["conditioning_indices"], strat)
        self.sc = HipScorer(sd, strategy=strat, seg_len=cfg["seg_len"], cond_idx=ci, corrupt_idx=xi,
                            cond_channels=list(cfg["channels"]) + [cfg["h_dim"]], device="cuda:0")
        self.L, self.h, self.strategy = self.sc.L, self.sc._h, strat
        dev = "cuda:0"
        self.data = torch.zeros(B, 2, cfg["seg_len"], 17, device=dev)
        self.table = self.sc.table(NS)
        self.ws = torch.zeros(1 << 22, dtype=torch.uint8, device=dev)
        self.loss = torch.zeros(B, S, device=dev)
        self.agg = torch.zeros(B, device=dev)
        self.mask = torch.full((B,), 3, dtype=torch.int32, device=dev)
        self.x = torch.zeros(B, 2, self.sc.t_unet, 17, device=dev)
        self.emb = torch.zeros(B, 16, device=dev)

    cfg = make_cfg

    def view(self, **kw):
        if self.strategy == "random_imp":
            kw.setdefault("cond_mask", self.mask.data_ptr())
        return view(**kw) if kw else None

    def fused(self, cfg="default", w="default", v="default", data="default", table="default", ws="default", aggr=1, q=0.0,
              agg="default", loss=None):
        d = lambda a, b: b if isinstance(a, str) else a
        cfg, v = d(cfg, self.cfg()), d(v, self.view())
        return self.L.mcd_score_fused(d(w, self.h), C.byref(cfg) if cfg is not None else None, d(data, _ptr(self.data)),
                                      C.byref(v) if v is not None else None, None, 1, 0, d(table, _ptr(self.table)), d(ws, _ptr(self.ws)),
                                      aggr, C.c_float(q), d(agg, _ptr(self.agg)), loss, None, None)

    def score_view(self, loss="default", v="default"):
        cfg, v = self.cfg(), self.view() if isinstance(v, str) else v
        return self.L.mcd_score_view(self.h, C.byref(cfg), _ptr(self.data), C.byref(v) if v is not None else None, None, 1, 0,
                                     _ptr(self.table), _ptr(self.ws), _ptr(self.loss) if isinstance(loss, str) else loss, None, None)

    def with_options(self, opts, fn):
        for k, val in opts.items():
            self.sc.set_option(k, val)
        try:
            return fn()
        finally:
            for k in opts:
                self.sc.set_option(k, 0)


def pose_cases(p: Pose):
    n_cond, n_cor, T = len(p.sc.cond_idx), len(p.sc.corrupt_idx), p.sc.seg_len
    c = {
        "null handle": lambda: p.fused(w=None),
        "null cfg": lambda: p.fused(cfg=None),
        "null data": lambda: p.fused(data=None),
        "null step_table": lambda: p.fused(table=None),
        "score_view: null loss_out": lambda: p.score_view(loss=None),
        "null loss_agg": lambda: p.fused(agg=None),
        "aggregation all": lambda: p.fused(aggr=0),
        "aggregation mean_pose": lambda: p.fused(aggr=5),
        "aggregation median_pose": lambda: p.fused(aggr=6),
        "aggregation 9": lambda: p.fused(aggr=9),
        "quantile 1.5": lambda: p.fused(aggr=7, q=1.5),
        "quantile nan": lambda: p.fused(aggr=7, q=NAN),
        "n_samples 0": lambda: p.fused(cfg=p.cfg(S=0)),
        "noise_steps 1": lambda: p.fused(cfg=p.cfg(ns=1)),
        "windows x samples over 2^31": lambda: p.fused(cfg=p.cfg(B=70000, S=70000)),
        "lists do not partition seg_len": lambda: p.fused(cfg=p.cfg(n_corrupt=n_cor - 1)),
        "n_corrupt 0": lambda: p.fused(cfg=p.cfg(n_corrupt=0, n_cond=T)),
        "seg_len 33": lambda: p.fused(cfg=p.cfg(seg_len=33, n_cond=33 - n_cor)),
        "cond_idx past the window": lambda: p.fused(cfg=p.cfg(cond_idx={0: T})),
        "corrupt_idx negative": lambda: p.fused(cfg=p.cfg(corrupt_idx={0: -1})),
        "trans without affine": lambda: p.fused(v=p.view(trans=p.mask.data_ptr())),
        "generic_unet, no workspace": lambda: p.with_options({"generic_unet": 1}, lambda: p.fused(ws=None)),
        "cond_encode: null handle": lambda: p.L.mcd_cond_encode(None, _ptr(p.data), B, _ptr(p.emb), None),
        "cond_encode: null cond_data": lambda: p.L.mcd_cond_encode(p.h, None, B, _ptr(p.emb), None),
        "unet_forward: null x": lambda: p.L.mcd_unet_forward(p.h, None, None, _ptr(p.table), 1, B, _ptr(p.x), None, None),
        "unet_forward: t -1": lambda: p.L.mcd_unet_forward(p.h, _ptr(p.x), None, _ptr(p.table), -1, B, _ptr(p.x), None, None),
        "unet_forward: generic_unet, no workspace": lambda: p.with_options(
            {"generic_unet": 1}, lambda: p.L.mcd_unet_forward(p.h, _ptr(p.x), None, _ptr(p.table), 1, B, _ptr(p.x), None, None)),
        "layer_forward: stage 15": lambda: p.L.mcd_layer_forward(p.h, 15, _ptr(p.x), None, _ptr(p.emb), B, _ptr(p.x), None, None),
        "layer_forward: skip": lambda: p.L.mcd_layer_forward(p.h, 1, _ptr(p.x), _ptr(p.x), _ptr(p.emb), B, _ptr(p.x), None, None),
        "set_option: 99": lambda: p.L.mcd_set_option(p.h, 99, 1),
        "plan_split: null cfg": lambda: p.L.mcd_plan_split(p.h, None),
    }
    # (only cases that the handle's strategy rejects: anything else would be a launch)
    if p.strategy == "inject":
        c["frame split moved"] = lambda: p.fused(cfg=p.cfg(n_cond=n_cond + 1, n_corrupt=n_cor - 1))
        c["n_cond differs from the packed encoder"] = lambda: p.fused(cfg=p.cfg(seg_len=T + 1, n_cond=n_cond + 1))
        c["split 2, no workspace"] = lambda: p.with_options({"split": 2}, lambda: p.fused(ws=None))
        c["cond_generic, no workspace"] = lambda: p.with_options({"cond_generic": 1, "split": 2}, lambda: p.fused(ws=None))
    else:
        c["frame split moved"] = lambda: p.fused(cfg=p.cfg(seg_len=T + 1, n_cond=n_cond + 1))
    if p.strategy == "concat":
        c["corrupt_idx twice"] = lambda: p.fused(cfg=p.cfg(corrupt_idx={1: p.sc.corrupt_idx[0]}))
    if p.strategy == "random_imp":
        c["no view"] = lambda: p.fused(v=None)
        c["view without cond_mask"] = lambda: p.fused(v=view())
        c["score_view: no view"] = lambda: p.score_view(v=None)
    return c


class Latent:
    def __init__(self, name="A_benign"):
        import latent_ref as R
        import latentt_fixtures as TT
        from helpers import make_args
        from mocodad_amd.models.mocodad_latent import MoCoDADlatent
        sd, _, cfg, _ = TT.load(name) if name in TT.NAMES else R.load_fixture(name)
        m = MoCoDADlatent(make_args(cfg))
        m.load_state_dict(sd, strict=False)
        self.sc = m.to("cuda:0").scorer()
        self.L, self.h, D = self.sc.L, self.sc._h, self.sc.latent_dim
        dev = "cuda:0"
        self.data = torch.zeros(B, 2, self.sc.seg_len, 17, device=dev)
        self.table = self.sc.table(NS)
        self.ws = torch.zeros(1 << 20, dtype=torch.uint8, device=dev)
        self.loss = torch.zeros(B, S, device=dev)
        self.agg = torch.zeros(B, device=dev)
        self.noise = torch.zeros(S * (NS - 1) * B * D + 4, device=dev)
        self.z = torch.zeros(B, D + 4, device=dev)
        self.emb = torch.zeros(B, 16, device=dev)
        self.i32 = torch.zeros(B, dtype=torch.int32, device=dev)

    cfg = make_cfg

    def score(self, cfg="default", w="default", v=None, data="default", table="default", ws="default", noise=None, aggr=1, q=0.0,
              agg="default", loss=None):
        d = lambda a, b: b if isinstance(a, str) else a
        cfg = d(cfg, self.cfg())
        return self.L.mcd_latent_score(d(w, self.h), C.byref(cfg) if cfg is not None else None, d(data, _ptr(self.data)),
                                       C.byref(v) if v is not None else None, noise, 1, 0, d(table, _ptr(self.table)), d(ws, _ptr(self.ws)),
                                       aggr, C.c_float(q), d(agg, _ptr(self.agg)), loss, None, None, None)

    def encode(self, cfg="default", data="default", cond="default", z_off=0):
        d = lambda a, b: b if isinstance(a, str) else a
        cfg = d(cfg, self.cfg())
        return self.L.mcd_latent_encode(self.h, C.byref(cfg), d(data, _ptr(self.data)), None, _ptr(self.table), d(cond, _ptr(self.emb)),
                                        _ptr(self.z, z_off), None)

    def denoise(self, x="default", t=1, off=0):
        return self.L.mcd_latent_denoise(self.h, _ptr(self.z, off) if isinstance(x, str) else x, _ptr(self.emb), _ptr(self.table), t, B,
                                         _ptr(self.noise), None)


def latent_cases(p: Latent):
    n_cond, n_cor, T = len(p.sc.cond_idx), len(p.sc.corrupt_idx), p.sc.seg_len
    return {
        "null handle": lambda: p.score(w=None),
        "null cfg": lambda: p.score(cfg=None),
        "null data": lambda: p.score(data=None),
        "null step_table": lambda: p.score(table=None),
        "no workspace": lambda: p.score(ws=None),
        "all, null loss_all": lambda: p.score(aggr=0),
        "null loss_agg": lambda: p.score(agg=None),
        "aggregation mean_pose": lambda: p.score(aggr=5),
        "aggregation 9": lambda: p.score(aggr=9),
        "quantile 1.5": lambda: p.score(aggr=7, q=1.5),
        "quantile nan": lambda: p.score(aggr=7, q=NAN),
        "n_samples 0": lambda: p.score(cfg=p.cfg(S=0)),
        "noise_steps 1": lambda: p.score(cfg=p.cfg(ns=1)),
        "n_samples 1025": lambda: p.score(cfg=p.cfg(S=1025)),
        "windows x samples over 2^31": lambda: p.score(cfg=p.cfg(B=1 << 22, S=1024)),
        "loss_fn 7": lambda: p.score(cfg=p.cfg(loss_fn=7)),
        "misaligned noise": lambda: p.score(noise=_ptr(p.noise, 4)),
        "misaligned workspace": lambda: p.score(ws=_ptr(p.ws, 8)),
        "trans without affine": lambda: p.score(v=view(trans=p.i32.data_ptr())),
        "frame split moved": lambda: p.score(cfg=p.cfg(n_cond=n_cond + 1, n_corrupt=n_cor - 1)),
        "lists do not partition seg_len": lambda: p.score(cfg=p.cfg(seg_len=T + 1)),
        "cond_idx past the window": lambda: p.score(cfg=p.cfg(cond_idx={0: T})),
        "corrupt_idx negative": lambda: p.score(cfg=p.cfg(corrupt_idx={0: -1})),
        "trans without affine and a bad index": lambda: p.score(v=view(trans=p.i32.data_ptr()), cfg=p.cfg(cond_idx={0: T})),
        "encode: null data": lambda: p.encode(data=None),
        "encode: null cond_emb_out": lambda: p.encode(cond=None),
        "encode: noise_steps 1": lambda: p.encode(cfg=p.cfg(ns=1)),
        "encode: frame split moved": lambda: p.encode(cfg=p.cfg(n_cond=n_cond + 1, n_corrupt=n_cor - 1)),
        "encode: corrupt_idx past the window": lambda: p.encode(cfg=p.cfg(corrupt_idx={2: T})),
        "denoise: null x": lambda: p.denoise(x=None),
        "denoise: t -1": lambda: p.denoise(t=-1),
        "denoise: misaligned x": lambda: p.denoise(off=4),
        "set_option: 9": lambda: p.L.mcd_latent_set_option(p.h, 9, 1),
    }


def latent_s12_cases(p: Latent):
    """6 + 6 frames: at 5 .. 12 corrupt frames latent_project_kernel stores z0 four floats at a time (at 3 the encode launch stores
    single floats and takes any float alignment: nothing to reject there)."""
    return {
        "encode: misaligned z0_out": lambda: p.encode(z_off=4),
    }


HANDLES = ["inject", "concat", "rndimp", "latent", "latentS12"]


def cases(handle):
    if handle not in _ctx:
        if handle == "latentS12":
            _ctx[handle] = latent_s12_cases(Latent("S12"))
        else:
            p = Latent() if handle == "latent" else Pose(handle)
            _ctx[handle] = latent_cases(p) if handle == "latent" else pose_cases(p)
    return _ctx[handle]


def run_all(handle):
    L = _lib.lib()
    out = {}
    for name, fn in cases(handle).items():
        out[name] = run_case(L, lambda _L: fn())
    torch.cuda.synchronize()        # (nothing was launched: a fault of an earlier call would surface here)
    return out


@pytest.mark.parametrize("handle", HANDLES)
def test_rejected_by_host_validation(handle):
    got, want = run_all(handle), expected("gpu")[handle]
    assert sorted(got) == sorted(want)
    for name in got:
        assert got[name][0] < 0, f"{name}: must be a rejected call"
        assert got[name] == want[name], name


if __name__ == "__main__":
    assert sys.argv[1:2] == ["--record"], __doc__
    res = {h: run_all(h) for h in HANDLES}
    bad = [(h, n) for h in res for n, (c, _) in res[h].items() if c >= 0]
    assert not bad, f"not rejected: {bad}"
    record("gpu", res, sys.argv[2] if len(sys.argv) > 2 else JSON)
    for h in res:
        for n, v in res[h].items():
            print(h, "|", n, "|", v)
