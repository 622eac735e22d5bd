#!/usr/bin/env python3
"""Generate the forecast-track fixture by IMPORTING the reference (aleflabo/MoCoDAD) on CPU.

    python tests/golden/gen_forecast_golden.py        (needs a checkout of the reference: MOCODAD_REFERENCE=<path>)

Writes tests/golden/forecast_tracks.npz: for nine persons -- Tx in {1, 3, 12} forecast frames behind 3 condition frames, forecasts
scaled by 0.01, 1 and 5, every track with a jump in its frame ids -- the stride-1 windows' forecasts `pos` (w, 2, Tx, 17) fp32 and
the 1-based frame ids `frames_pos` (w, Tx) of their forecast frames, and what the reference's compute_fig_matrix +
extract_single_pose (utils/eval_utils.py:13-24, 37-72) make of them: `single_<method>` (n_frames, 34) f64 for unique / mean /
median, `std_<std_method>` (n_frames,) f64 = its std_vec for mean / median (taken with std_lift = 0 and the MinMaxScaler of the
reference module's namespace replaced by an identity while the function runs -- the only way to see the vector before the MinMax
step) and `score_<std_method>` (n_frames,) f64 = its std_score as returned.  A frame is covered by 1 .. Tx windows: cover counts
1, 2, 3 and every even and odd count up to 12.  No forecast row sums to exactly 0 (asserted): the reference finds "absent" by
`!= 0`.  Only DATA is written; no reference source text is stored."""
import os
import sys

import numpy as np

REF = os.environ.get("MOCODAD_REFERENCE")
HERE = os.path.dirname(os.path.abspath(__file__))
N_COND = 3
ROWS = 30          # rows of a track; the frame ids jump by 5 behind row 13


class _Identity:
    def fit_transform(self, x):
        return x


def main():
    if not REF or not os.path.isdir(REF):
        raise SystemExit("set MOCODAD_REFERENCE to a checkout of the reference (aleflabo/MoCoDAD)")
    sys.path.insert(0, REF)
    import utils.eval_utils as ref
    out = {"sklearn": np.asarray(__import__("sklearn").__version__), "numpy": np.asarray(np.__version__)}
    person = 0
    for Tx in (1, 3, 12):
        for scale in (0.01, 1.0, 5.0):
            rng = np.random.default_rng(1000 + person)
            seg_len = N_COND + Tx
            ids = np.arange(1, ROWS + 1) + 2 * person
            ids[14:] += 5
            w = ROWS - seg_len + 1
            pos = (rng.normal(0, 1, (w, 2, Tx, 17)) * scale).astype(np.float32)
            frames_pos = np.stack([ids[s + N_COND:s + seg_len] for s in range(w)]).astype(np.int32)
            n_frames = int(ids.max())
            assert (pos.transpose(0, 2, 3, 1).reshape(w, Tx, 34).astype(np.float64).sum(-1) != 0).all()
            fig = ref.compute_fig_matrix(pos, frames_pos, n_frames)
            p = f"p{person}_"
            out[p + "pos"], out[p + "frames_pos"], out[p + "n_frames"] = pos, frames_pos, np.asarray(n_frames)
            for method in ("unique", "mean", "median"):
                single, _ = ref.extract_single_pose(fig, method=method, std=True, std_method="mean")
                out[p + "single_" + method] = single
            for std_method in ("mean", "median"):
                _, score = ref.extract_single_pose(fig, method="median", std=True, std_method=std_method)
                keep, ref.MinMaxScaler = ref.MinMaxScaler, _Identity
                try:
                    _, vec = ref.extract_single_pose(fig, method="median", std=True, std_method=std_method, std_lift=0.0)
                finally:
                    ref.MinMaxScaler = keep
                out[p + "std_" + std_method], out[p + "score_" + std_method] = np.asarray(vec, np.float64), np.asarray(score, np.float64)
            person += 1
    out["n_persons"] = np.asarray(person)
    np.savez_compressed(os.path.join(HERE, "forecast_tracks.npz"), **out)
    print("wrote forecast_tracks.npz:", person, "persons")


if __name__ == "__main__":
    main()
