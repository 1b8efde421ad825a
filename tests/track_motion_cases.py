"""Frame pairs for Tracking::TrackWithMotionModel (src/Tracking.cpp:724-774) (TEST-ONLY), shared by
tests/test_cpu_track_motion.py and tests/test_gpu_track_motion.py: one current Frame observing the MapPoints
of the last Frame's slots, with a predicted pose (mVelocity * mLastFrame.mTcw) that is the true pose turned by
`yaw` about the camera's y axis, which moves every projection by about fx * yaw pixels."""
from __future__ import annotations

import types

import numpy as np

import lastproj_cases as lc
from rsc import synth

f32 = np.float32
TH = 7.0   # the stereo threshold (:731)


def make_pair(seed: int, n: int, yaw: float, n_wrong: int = 0, no_obs_frac: float = 0.0, n_extra: int = 60):
    """n LastFrame slots whose MapPoints the current Frame observes, plus n_extra unrelated features and slots.
    n_wrong slots carry a MapPoint 5 sigma beside its feature: inside the search window, so matched by the
    descriptor, and an outlier of the pose optimisation."""
    rng = np.random.default_rng(seed)
    fx, fy, cx, cy = (float(v) for v in (synth.FX, synth.FY, synth.CX, synth.CY))
    W, H, mbf = float(synth.WIDTH), float(synth.HEIGHT), float(synth.EUROC_BF)
    sf = synth.scale_factors().astype(np.float64)
    m = n + n_extra
    uv = np.stack([rng.uniform(60, W - 60, m), rng.uniform(60, H - 60, m)], 1)
    z = rng.uniform(3, 9, m)
    octave = rng.integers(0, 4, m).astype(np.int32)
    angle = rng.uniform(0, 360, m)
    desc = rng.integers(0, 256, (m, 32), dtype=np.uint8)
    R, t = synth.random_rotation(rng, 0.1), rng.uniform(-0.3, 0.3, 3)
    # the MapPoints: behind the features, the wrong ones 5 sigma to the side; the extra slots anywhere
    src = uv.copy()
    wrong = rng.choice(n, n_wrong, replace=False)
    d = rng.normal(size=(n_wrong, 2))
    src[wrong] += 5.0 * sf[octave[wrong], None] * d / np.linalg.norm(d, axis=1, keepdims=True)
    src[n:] = np.stack([rng.uniform(60, W - 60, n_extra), rng.uniform(60, H - 60, n_extra)], 1)
    Pc = np.stack([(src[:, 0] - cx) / fx * z, (src[:, 1] - cy) / fy * z, z], 1)
    pos = (Pc - t) @ R
    kp = uv + rng.normal(0, 0.3, (m, 2))
    u_right = np.where(rng.random(m) < 0.5, kp[:, 0] - mbf / z + rng.normal(0, 0.3, m), -1.0).astype(f32)
    fr = lc.make_frame(kp, octave, desc, u_right, mbf=mbf)
    fr.angle = angle.astype(f32)
    sdesc = np.array([lc._flip(rng, desc[i], 6) for i in range(m)])
    sdesc[n:] = rng.integers(0, 256, (n_extra, 32), dtype=np.uint8)
    state = np.where(rng.random(m) < 0.05, rng.integers(0, 2, m) * 2, 1).astype(np.uint8)
    has_obs = (rng.random(m) >= no_obs_frac).astype(np.uint8)
    last = lc.last_of(octave, (angle + rng.normal(0, 3, m)) % 360.0, state, pos, sdesc, has_obs)
    Ry = np.array([[np.cos(yaw), 0, np.sin(yaw)], [0, 1, 0], [-np.sin(yaw), 0, np.cos(yaw)]])
    Tc, Tl = np.eye(4), np.eye(4)
    Tc[:3, :3], Tc[:3, 3] = Ry @ R, Ry @ t
    Tl[:3, :3], Tl[:3, 3] = R, t + np.array([0.0, 0.0, 0.05])
    return types.SimpleNamespace(frame=fr, last=last, Tcw_cur=Tc.astype(f32), Tcw_last=Tl.astype(f32),
                                 mb=float(f32(mbf / fx)), frame_occ=np.zeros(fr.n, np.uint8), th=TH, check_ori=1,
                                 wrong=np.sort(wrong))


def frames():
    """name -> (pair, only_tracking, what the replay must show).  fx * yaw: 0.9, 13 and 44 pixels (the largest
    radius at th is 7 * 1.728 = 12.1)."""
    return {
        "at_th": (make_pair(41, 300, 0.002), 0, dict(ok=1, searches=1)),
        "at_2th": (make_pair(42, 300, 0.03), 0, dict(ok=1, searches=2)),
        "fails": (make_pair(43, 300, 0.1), 0, dict(ok=0, searches=2)),
        "outliers": (make_pair(44, 400, 0.002, n_wrong=40, no_obs_frac=0.3), 0, dict(ok=1, searches=1)),
        "only_tracking_vo": (make_pair(45, 300, 0.002, no_obs_frac=0.985), 1, dict(ok=1, searches=1, vo=1)),
        "small": (make_pair(46, 12, 0.002, n_extra=4), 1, dict(ok=0, searches=2)),
    }
