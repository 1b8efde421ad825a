"""Hand-built frames for Frame::ComputeStereoMatches() with their expected outputs written out literally (worked by
hand from src/Frame.cpp:538-673, not taken from stereo_ref).  TEST-ONLY.

Every case uses mbf = 40, mb = 0.5 (maxD = 80) and scale factors 1.2^l.  A left descriptor is all zeros and right
keypoint j carries `d` set bits, so its distance to every left keypoint is d.  Left entries are (u, y, octave),
right entries (u, y, octave, d).  At octave 0 the row window is yL - 2 < yR <= yL + 2."""
from __future__ import annotations

import numpy as np

import stereo_ref as sr

MBF, MB = 40.0, 0.5
N_LEVELS = 8


def scale_factors():
    s = np.ones(N_LEVELS, np.float32)
    for l in range(1, N_LEVELS):  # ORBextractor: mvScaleFactor[i] = mvScaleFactor[i-1] * scaleFactor
        s[l] = np.float32(s[l - 1] * np.float32(1.2))
    return s


def bits(d: int):
    """A 32-byte descriptor with d set bits."""
    v = np.zeros(256, np.uint8)
    v[:d] = 1
    return np.packbits(v)


def build(left, right):
    kp = [(u, y) for u, y, _ in left]
    octave = [o for _, _, o in left]
    desc = np.zeros((len(left), 32), np.uint8)
    r_kp = [(u, y) for u, y, _, _ in right]
    r_oct = [o for _, _, o, _ in right]
    r_desc = np.array([bits(d) for _, _, _, d in right], np.uint8).reshape(-1, 32)
    return sr.frame(kp, octave, desc, scale_factors(), r_kp, r_oct, r_desc, MBF, MB)


NONE = dict(u_right=[-1.0], depth=[-1.0], best_right=[-1], best_dist=[-1], n_candidates=0, n_removed=0, median=-1)
TH_NONE = -2.0999999046325684  # 1.5f * 1.4f * -1; 2.1f = 8808038 * 2^-22, so 2.1f * 5 is a tie that rounds to 10.5

# (name, left, right, expected)
CASES = [
    # yR == yL - r is outside the window, yR == yL + r inside: the far worse keypoint on the upper edge wins
    ("window_edges", [(100.0, 50.0, 0)], [(90.0, 48.0, 0, 5), (80.0, 52.0, 0, 30)],
     dict(u_right=[80.0], depth=[2.0], best_right=[1], best_dist=[30], n_candidates=1, n_removed=0, median=30,
          th_dist=62.999996185302734)),
    ("lower_edge_only", [(100.0, 50.0, 0)], [(90.0, 48.0, 0, 5)], dict(NONE, th_dist=TH_NONE)),
    ("just_above_upper_edge", [(100.0, 50.0, 0)], [(90.0, 52.000004, 0, 5)], dict(NONE, th_dist=TH_NONE)),
    # uR == minU = 20 passes the u gate and wins on distance; its disparity == maxD = 80 fails `< maxD`, so the
    # keypoint ends without a match although right 1 would have been acceptable
    ("u_at_min_u_disparity_at_max_d", [(100.0, 50.0, 0)], [(20.0, 50.0, 0, 5), (50.0, 50.0, 0, 10)],
     dict(NONE, th_dist=TH_NONE)),
    # just inside: uR = 20.00001f = 20.0000095..., disparity rounds to 79.99999237 < 80 (20.000002f would round to 80)
    ("u_just_above_min_u", [(100.0, 50.0, 0)], [(20.00001, 50.0, 0, 5), (50.0, 50.0, 0, 10)],
     dict(u_right=[20.000009536743164], depth=[0.5000000596046448], best_right=[0], best_dist=[5], n_candidates=1,
          n_removed=0, median=5, th_dist=10.5)),
    # uR == maxU = uL: disparity 0 becomes (float)0.01, mvuRight = (float)((double)uL - 0.01)
    ("u_at_max_u_zero_disparity", [(100.0, 50.0, 0)], [(100.0, 50.0, 0, 5), (100.00001, 50.0, 0, 1)],
     dict(u_right=[99.98999786376953], depth=[4000.0], best_right=[0], best_dist=[5], n_candidates=1, n_removed=0,
          median=5, th_dist=10.5)),
    # uL = 0.01f: the double subtraction leaves -2.2e-10 where a float subtraction would leave 0
    ("zero_disparity_double_subtraction", [(0.01, 50.0, 0)], [(0.01, 50.0, 0, 5)],
     dict(u_right=[-2.2351741291171123e-10], depth=[4000.0], best_right=[0], best_dist=[5], n_candidates=1,
          n_removed=0, median=5, th_dist=10.5)),
    # maxU < 0 skips the keypoint before any search; uL = 0 is not skipped
    ("max_u_negative", [(-0.5, 50.0, 0)], [(-0.5, 50.0, 0, 0), (-1.0, 50.0, 0, 0)], dict(NONE, th_dist=TH_NONE)),
    ("max_u_zero", [(0.0, 50.0, 0)], [(0.0, 50.0, 0, 7)],
     dict(u_right=[-0.009999999776482582], depth=[4000.0], best_right=[0], best_dist=[7], n_candidates=1, n_removed=0,
          median=7, th_dist=14.69999885559082)),
    # left octave 2 (r = 2.88): octaves 0 and 4 are out whatever their distance, 1 and 3 are in
    ("octave_gate", [(100.0, 50.0, 2)],
     [(90.0, 50.0, 0, 1), (90.0, 50.0, 4, 2), (90.0, 50.0, 1, 20), (60.0, 50.0, 3, 10)],
     dict(u_right=[60.0], depth=[1.0], best_right=[3], best_dist=[10], n_candidates=1, n_removed=0, median=10,
          th_dist=21.0)),
    # equal distances in two rows: the smaller y comes first in sorted order and keeps the strict <
    ("tie_between_rows", [(100.0, 50.0, 0)], [(90.0, 51.0, 0, 10), (60.0, 49.5, 0, 10)],
     dict(u_right=[60.0], depth=[1.0], best_right=[1], best_dist=[10], n_candidates=1, n_removed=0, median=10,
          th_dist=21.0)),
    # equal distances inside one row: the smaller index
    ("tie_inside_row", [(100.0, 50.0, 0)], [(95.0, 50.0, 0, 12), (90.0, 50.0, 0, 10), (60.0, 50.0, 0, 10)],
     dict(u_right=[90.0], depth=[4.0], best_right=[1], best_dist=[10], n_candidates=1, n_removed=0, median=10,
          th_dist=21.0)),
    # +0.0f and -0.0f are one row: index 0 wins although -0.0f has the smaller bit-pattern order
    ("tie_across_signed_zero", [(100.0, 0.5, 0)], [(90.0, 0.0, 0, 10), (60.0, -0.0, 0, 10)],
     dict(u_right=[90.0], depth=[4.0], best_right=[0], best_dist=[10], n_candidates=1, n_removed=0, median=10,
          th_dist=21.0)),
    ("tie_across_signed_zero_swapped", [(100.0, 0.5, 0)], [(90.0, -0.0, 0, 10), (60.0, 0.0, 0, 10)],
     dict(u_right=[90.0], depth=[4.0], best_right=[0], best_dist=[10], n_candidates=1, n_removed=0, median=10,
          th_dist=21.0)),
    # bestDist < 75: 74 is accepted, 75 is not
    ("distance_74_and_75", [(100.0, 10.0, 0), (100.0, 30.0, 0)], [(60.0, 10.0, 0, 74), (60.0, 30.0, 0, 75)],
     dict(u_right=[60.0, -1.0], depth=[1.0, -1.0], best_right=[0, -1], best_dist=[74, -1], n_candidates=1,
          n_removed=0, median=74, th_dist=155.39999389648438)),
    # bestDist starts at TH_HIGH: nothing at or above 100 is ever the best
    ("distance_100", [(100.0, 10.0, 0)], [(60.0, 10.0, 0, 100), (60.0, 10.0, 0, 256)], dict(NONE, th_dist=TH_NONE)),
    # median 0: thDist = 0 and `0 < 0` is false, so every match goes
    ("median_zero_removes_all", [(100.0, 10.0, 0), (100.0, 30.0, 0), (100.0, 50.0, 0)],
     [(60.0, 10.0, 0, 0), (80.0, 30.0, 0, 0), (90.0, 50.0, 0, 0)],
     dict(u_right=[-1.0, -1.0, -1.0], depth=[-1.0, -1.0, -1.0], best_right=[0, 1, 2], best_dist=[0, 0, 0],
          n_candidates=3, n_removed=3, median=0, th_dist=0.0)),
    # distances 5, 10, 10, 20, 21: median = element 2 = 10, thDist = 2.1f * 10 rounds to 21.0f; 21 goes, 20 stays
    ("median_10_cuts_21_keeps_20",
     [(100.0, 10.0, 0), (100.0, 30.0, 0), (100.0, 50.0, 0), (100.0, 70.0, 0), (100.0, 90.0, 0)],
     [(60.0, 10.0, 0, 21), (60.0, 30.0, 0, 10), (60.0, 50.0, 0, 20), (60.0, 70.0, 0, 5), (60.0, 90.0, 0, 10)],
     dict(u_right=[-1.0, 60.0, 60.0, 60.0, 60.0], depth=[-1.0, 1.0, 1.0, 1.0, 1.0], best_right=[0, 1, 2, 3, 4],
          best_dist=[21, 10, 20, 5, 10], n_candidates=5, n_removed=1, median=10, th_dist=21.0)),
    # an even count takes the upper of the two middle elements: 4, 8 -> vDistIdx[1] = 8
    ("median_of_two", [(100.0, 10.0, 0), (100.0, 30.0, 0)], [(60.0, 10.0, 0, 8), (60.0, 30.0, 0, 4)],
     dict(u_right=[60.0, 60.0], depth=[1.0, 1.0], best_right=[0, 1], best_dist=[8, 4], n_candidates=2, n_removed=0,
          median=8, th_dist=16.799999237060547)),
    ("empty_right", [(100.0, 10.0, 0), (100.0, 30.0, 0)], [],
     dict(u_right=[-1.0, -1.0], depth=[-1.0, -1.0], best_right=[-1, -1], best_dist=[-1, -1], n_candidates=0,
          n_removed=0, median=-1, th_dist=TH_NONE)),
    ("empty_left", [], [(60.0, 10.0, 0, 0)],
     dict(u_right=[], depth=[], best_right=[], best_dist=[], n_candidates=0, n_removed=0, median=-1, th_dist=TH_NONE)),
    ("empty_both", [], [],
     dict(u_right=[], depth=[], best_right=[], best_dist=[], n_candidates=0, n_removed=0, median=-1, th_dist=TH_NONE)),
]


def cases():
    """[(name, frame, expected result dict in the form of stereo_ref.compute)]."""
    out = []
    for name, left, right, exp in CASES:
        e = dict(exp)
        e["u_right"] = np.array(exp["u_right"], np.float64).astype(np.float32)
        e["depth"] = np.array(exp["depth"], np.float64).astype(np.float32)
        e["best_right"] = np.array(exp["best_right"], np.int32)
        e["best_dist"] = np.array(exp["best_dist"], np.int32)
        e["th_dist"] = np.float32(exp["th_dist"])
        out.append((name, build(left, right), e))
    return out


# ---- random frames (tests/golden/make_stereo_golden.py writes their expected outputs) ----
# name: (seed, left keypoints, right keypoints, integer-pixel y).  Right sizes stand one below, at and one above
# the kernel's strides: a wave's 64 lanes, the workgroup's 256 staging lanes, the LDS chunk of 2,048 (4,097: a third
# chunk).  Left sizes end a tile of 32 and a wave's 8 in every way (1, 63, 64, 65, 200, 1,200).
RANDOM_FRAMES = {
    "r_1x63": (11, 1, 63, False), "r_63x64": (12, 63, 64, False), "r_64x65": (13, 64, 65, True),
    "r_63x255": (14, 63, 255, True), "r_64x256": (15, 64, 256, False), "r_65x257": (16, 65, 257, True),
    "r_65x2047": (17, 65, 2047, False), "r_200x2048": (18, 200, 2048, True), "r_200x2049": (19, 200, 2049, False),
    "r_200x4097": (20, 200, 4097, True), "r_1200x1300": (21, 1200, 1300, False),
}
R_MBF, R_MB = 47.90639384423901, 47.90639384423901 / 458.654  # EuRoC: maxD = fx


def random_frame(seed: int, n: int, m: int, integer_y: bool):
    """A left frame of n keypoints and a right frame of m: min(n, m) right keypoints are partners of a left one (a
    row within +-1, a disparity in [0, 200], exactly 0 for one in twenty, an octave within +-1, 3 to 73 flipped
    descriptor bits), a few are copies of a partner in the same row or the next one (distance ties), the rest are
    unrelated.  The right frame is shuffled."""
    rng = np.random.default_rng(seed)
    kp = np.empty((n, 2), np.float32)
    kp[:, 0] = rng.uniform(0.0, 752.0, n)
    kp[:, 1] = rng.uniform(0.0, 480.0, n)
    if integer_y:
        kp[:, 1] = np.floor(kp[:, 1])
    octave = rng.choice(N_LEVELS, n, p=[0.3, 0.2, 0.15, 0.1, 0.1, 0.05, 0.05, 0.05]).astype(np.int32)
    desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    n_par = min(n, m)
    n_same = min((m - n_par) // 4, max(n_par // 8, 1)) if m > n_par else 0
    n_next = n_same
    r_kp = np.empty((m, 2), np.float32)
    r_oct = np.empty(m, np.int32)
    r_desc = np.empty((m, 32), np.uint8)
    owners = rng.permutation(n)[:n_par]
    for j, i in enumerate(owners):
        disp = 0.0 if rng.random() < 0.05 else rng.uniform(0.0, min(float(kp[i, 0]), 200.0))
        r_kp[j, 0] = np.float32(kp[i, 0] - np.float32(disp))
        dy = float(rng.integers(-1, 2)) if integer_y else rng.uniform(-1.0, 1.0)
        r_kp[j, 1] = np.float32(kp[i, 1] + np.float32(dy))
        r_oct[j] = min(max(int(octave[i]) + int(rng.integers(-1, 2)), 0), N_LEVELS - 1)
        k = int(rng.integers(3, 30)) if rng.random() < 0.85 else int(rng.integers(30, 74))
        flip = np.zeros(256, np.uint8)
        flip[rng.choice(256, k, replace=False)] = 1
        r_desc[j] = desc[i] ^ np.packbits(flip)
    for t in range(n_same + n_next):  # copies of a partner: the same row, or the next row up
        j, src = n_par + t, int(rng.integers(0, n_par))
        r_kp[j] = r_kp[src]
        if t < n_same:
            r_kp[j, 0] = np.float32(r_kp[src, 0] - np.float32(1.0))
        else:
            r_kp[j, 1] = np.float32(r_kp[src, 1] + np.float32(1.0))
        r_oct[j], r_desc[j] = r_oct[src], r_desc[src]
    rest = m - n_par - n_same - n_next
    a = n_par + n_same + n_next
    r_kp[a:, 0] = rng.uniform(0.0, 752.0, rest)
    r_kp[a:, 1] = np.floor(rng.uniform(0.0, 480.0, rest)) if integer_y else rng.uniform(0.0, 480.0, rest)
    r_oct[a:] = rng.integers(0, N_LEVELS, rest)
    r_desc[a:] = rng.integers(0, 256, (rest, 32), dtype=np.uint8)
    order = rng.permutation(m)
    return sr.frame(kp, octave, desc, scale_factors(), r_kp[order], r_oct[order], r_desc[order], R_MBF, R_MB)


def random_frames():
    return {name: random_frame(*spec) for name, spec in RANDOM_FRAMES.items()}


def digest(fr):
    """Sums over a frame's inputs: what the golden fixture keeps of a random frame."""
    return np.array([fr.kp.astype(np.float64).sum(), fr.r_kp.astype(np.float64).sum(), fr.octave.sum(),
                     fr.r_octave.sum(), fr.desc.astype(np.int64).sum(), fr.r_desc.astype(np.int64).sum()], np.float64)


def traits(fr, res):
    """What a result exercises, from the frame and a result of stereo_ref.compute alone: the accepted matches with
    disparity exactly 0, and those whose winner shared its distance with another candidate of the same row
    (the smaller index won) or of another row (the smaller y won)."""
    zero = same_row = other_row = 0
    max_d = np.float32(fr.mbf) / np.float32(fr.mb)
    for i in np.flatnonzero(res["best_right"] >= 0):
        j = int(res["best_right"][i])
        zero += int(fr.r_kp[j, 0] == fr.kp[i, 0])
        level = int(fr.octave[i])
        r = np.float32(2.0) * fr.scale[level]
        lo, hi = fr.kp[i, 1] - r, fr.kp[i, 1] + r
        ok = (fr.r_kp[:, 1] > lo) & (fr.r_kp[:, 1] <= hi) & (np.abs(fr.r_octave - level) <= 1) & \
            (fr.r_kp[:, 0] >= fr.kp[i, 0] - max_d) & (fr.r_kp[:, 0] <= fr.kp[i, 0])
        for k in np.flatnonzero(ok):
            if k != j and sr.descriptor_distance(fr.desc[i], fr.r_desc[k]) == int(res["best_dist"][i]):
                if fr.r_kp[k, 1] == fr.r_kp[j, 1]:
                    same_row += 1
                else:
                    other_row += 1
    return dict(zero_disparity=zero, tie_same_row=same_row, tie_other_row=other_row)
