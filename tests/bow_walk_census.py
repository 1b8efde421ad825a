"""ORBmatcher::SearchByBoW restated in numpy from the reference text (ORBmatcher.cpp:110-240 Frame
overload, :354-488 KeyFrame overload, ComputeThreeMaxima :1446-1487): a sequential walk per common
node over a per-node distance matrix, fast enough for inner nodes of thousands of features.  It
shares no code with orbmatch.hip or with the C oracle.

Besides the output vector and the match count it returns a *census* of what the inputs made the
reference do (per inner-node size class and segment count), and it can switch single rules off
(PERTURBATIONS) to show that a set of cases would notice an implementation that got the rule wrong.
The segment geometry used by the census and by perturbation (e) restates bow_segments()
(rsc_orbmatch.h): one segment per 64 inner positions, at most eight.
"""
import collections
import math

import numpy as np

TH_LOW = 50
HISTO_LENGTH = 30
MAX_SEGS = 8
STAGE = 256  # inner positions staged at a time by one wave of the distance kernel (kBowSeg)

PERTURBATIONS = {
    "a": "ignore the already-matched exclusion",
    "b": "never rescan: d2 = 256 when fewer than two of the four nearest valid positions are free",
    "c": "swap strict and inclusive TH_LOW between the overloads",
    "d": "last minimum wins first-minimum ties",
    "e": "second minimum taken only from the segment that holds the first minimum",
    "f": "invalid inner features not excluded (KeyFrame overload)",
    "g": "ratio test evaluated in double",
    "h": "no 10 % rule in ComputeThreeMaxima",
}

SIZE_CLASSES = ("<=64", "65-256", "257-512", ">512", ">2048")
FIELDS = ("candidates", "accepted", "rej_ratio", "rej_thresh", "rescan", "stolen", "d49_50", "near_ratio", "ties")


def segments(nb):
    return max(1, min(MAX_SEGS, (nb + 63) // 64))


def segment_length(nb):
    s = segments(nb)
    return (nb + s - 1) // s


def size_class(nb):
    if nb <= 64:
        return "<=64"
    if nb <= 256:
        return "65-256"
    if nb <= 512:
        return "257-512"
    return ">512" if nb <= 2048 else ">2048"


def distances(da, db):
    """Hamming distances int32[len(da), len(db)] of uint8[.,32] descriptor rows."""
    a = np.unpackbits(np.ascontiguousarray(da, np.uint8), axis=1).astype(np.float32)
    b = np.unpackbits(np.ascontiguousarray(db, np.uint8), axis=1).astype(np.float32)
    return (a @ (1.0 - b).T + (1.0 - a) @ b.T).astype(np.int32)  # exact: every sum is <= 256


def rot_bin(angle_a, angle_b):
    """:187-195 / :437-445 with the reference's factor 1.0f / HISTO_LENGTH."""
    rot = np.float32(np.float32(angle_a) - np.float32(angle_b))
    if rot < 0.0:
        rot = np.float32(rot + np.float32(360.0))
    x = float(np.float32(rot * (np.float32(1.0) / np.float32(HISTO_LENGTH))))
    b = int(math.floor(x + 0.5))  # round() of a non-negative value
    return 0 if b == HISTO_LENGTH else b


def three_maxima(sizes, ten_percent_rule=True):
    max1 = max2 = max3 = 0
    i1 = i2 = i3 = -1
    for i, s in enumerate(sizes):
        if s > max1:
            max3, max2, max1 = max2, max1, s
            i3, i2, i1 = i2, i1, i
        elif s > max2:
            max3, max2 = max2, s
            i3, i2 = i2, i
        elif s > max3:
            max3, i3 = s, i
    if ten_percent_rule:
        if np.float32(max2) < np.float32(0.1) * np.float32(max1):
            i2 = i3 = -1
        elif np.float32(max3) < np.float32(0.1) * np.float32(max1):
            i3 = -1
    return i1, i2, i3


def ratio_passes(d1, d2, ratio32, in_double=False):
    """(float)bestDist1 < mfNNratio * (float)bestDist2 (:181 / :432); mfNNratio is a float."""
    if in_double:
        return float(d1) < float(ratio32) * float(d2)
    return bool(np.float32(d1) < np.float32(ratio32) * np.float32(d2))


def walk(frame_variant, A, B, nnratio=0.75, check=True, perturb=""):
    """SearchByBoW(pKF = A, F = B) if frame_variant else SearchByBoW(pKF1 = A, pKF2 = B): A's
    features are taken in turn (outer), B's are searched (inner).  Returns (nmatches, out int32,
    census) with census[(size class, segments)] a Counter over FIELDS."""
    ratio32 = np.float32(nnratio)
    inclusive = frame_variant != ("c" in perturb)
    out = np.full(B.n if frame_variant else A.n, -1, np.int32)
    census = collections.defaultdict(collections.Counter)
    hist = [[] for _ in range(HISTO_LENGTH)]
    nm = 0
    _, ia, ib = np.intersect1d(A.node_id, B.node_id, return_indices=True)  # ascending node ids
    for ka, kb in zip(ia, ib):
        fa = A.feat[A.node_begin[ka]:A.node_begin[ka + 1]].astype(np.int64)
        fb = B.feat[B.node_begin[kb]:B.node_begin[kb + 1]].astype(np.int64)
        nb = len(fb)
        L = segment_length(nb)
        c = census[(size_class(nb), segments(nb))]
        D = distances(A.desc[fa], B.desc[fb])
        if frame_variant or B.valid is None or "f" in perturb:
            ok_b = np.ones(nb, bool)  # the Frame overload never looks at F's map points
        else:
            ok_b = B.valid[fb] != 0
        nvalid = int(ok_b.sum())
        # the four nearest valid positions of every outer feature in (distance, position) order
        keys = D.astype(np.int64) * 65536 + np.arange(nb)
        keys[:, ~ok_b] = np.iinfo(np.int64).max
        top4 = np.argsort(keys, axis=1, kind="stable")[:, :min(4, nvalid)]
        matched = np.zeros(nb, bool)
        for i, a in enumerate(fa):
            if A.valid is not None and not A.valid[a]:
                continue
            c["candidates"] += 1
            d = D[i]
            t4 = top4[i]
            free = np.flatnonzero(ok_b & ~matched)
            rescan = (nvalid > 4 and int(matched[t4].sum()) >= 3 and
                      (d[t4[0]] <= TH_LOW if frame_variant else d[t4[0]] < TH_LOW))
            c["rescan"] += int(rescan)
            b1, pos, b2 = 256, -1, 256
            if free.size:
                df = d[free]
                b1 = int(df.min())
                w = np.flatnonzero(df == b1)
                c["ties"] += int(w.size > 1 and b1 < 256)
                pos = int(free[w[-1] if "d" in perturb else w[0]])
                pool = df[free // L == pos // L] if "e" in perturb else df
                if pool.size >= 2:
                    b2 = min(256, int(np.partition(pool, 1)[1]))
                c["stolen"] += int(pos != t4[0])
            if "b" in perturb and rescan:
                f4 = t4[~matched[t4]]
                b1, pos, b2 = (int(d[f4[0]]), int(f4[0]), 256) if f4.size else (256, -1, 256)
            if b1 >= 256:
                pos = -1  # no distance ever beats the initial bestDist1 = 256
            c["d49_50"] += int(b1 in (49, 50))
            if not (b1 <= TH_LOW if inclusive else b1 < TH_LOW):
                c["rej_thresh"] += 1
                continue
            c["near_ratio"] += int(abs(b1 - float(ratio32) * b2) <= 1.0)
            if not ratio_passes(b1, b2, ratio32, "g" in perturb):
                c["rej_ratio"] += 1
                continue
            c["accepted"] += 1
            bi = int(fb[pos])
            if "a" not in perturb:
                matched[pos] = True
            if frame_variant:
                out[bi] = a  # vpMapPointMatches[bestIdxF] = pMP (:183)
                key = bi
            else:
                out[a] = bi  # vpMatches12[idx1] = vpMapPoints2[bestIdx2] (:434)
                key = a
            if check:
                hist[rot_bin(A.angle[a], B.angle[bi])].append(key)
            nm += 1
    if check:
        keep = three_maxima([len(h) for h in hist], "h" not in perturb)
        for i, h in enumerate(hist):
            if i in keep:
                continue
            for key in h:
                out[key] = -1
                nm -= 1
    return nm, out, census


def by_class(census):
    """Census summed over segment counts: {size class: Counter}."""
    tot = collections.defaultdict(collections.Counter)
    for (cls, _), c in census.items():
        tot[cls].update(c)
    return tot


def add(total, census):
    for k, c in census.items():
        total[k].update(c)
    return total


def table(total, title=""):
    """The census as text, one row per (size class, segment count)."""
    rows = [f"{title}", "class    segs " + " ".join(f"{f:>10}" for f in FIELDS)]
    for cls in SIZE_CLASSES:
        for (k, s) in sorted(x for x in total if x[0] == cls):
            rows.append(f"{k:<8} {s:>4} " + " ".join(f"{total[(k, s)][f]:>10}" for f in FIELDS))
    return "\n".join(rows)


# ---- float32 ratio arithmetic (the ratio-edge cases) -------------------------------------------
def ratio_equal_pairs(nnratio, dmax=TH_LOW):
    """Integer (d1, d2 <= dmax) with float32(d1) == float32(nnratio) * float32(d2)."""
    r = np.float32(nnratio)
    return [(d1, d2) for d2 in range(0, dmax + 1) for d1 in range(0, dmax + 1)
            if np.float32(d1) == r * np.float32(d2)]


def float_double_pairs(nnratio, d1max=TH_LOW - 1, d2max=256):
    """(d1, d2) where the float32 and the double product of the same operands put the ratio test on
    different sides of d1."""
    r = np.float32(nnratio)
    return [(d1, d2) for d2 in range(1, d2max + 1) for d1 in range(0, d1max + 1)
            if ratio_passes(d1, d2, r, False) != ratio_passes(d1, d2, r, True)]
