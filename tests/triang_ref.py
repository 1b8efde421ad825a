"""Sequential numpy-float32 restatement of LocalMapping::CreateNewMapPoints' matcher and geometry (TEST-ONLY):
ORBmatcher::SearchForTriangulation (src/ORBmatcher.cpp:489-669), the pair geometry and the neighbour loop
(src/LocalMapping.cpp:224-428), ComputeF12 (:512-531).  Literal loops, float32 scalars, sums left to right; the
neighbour loop fills slots as it goes (no speculation).  Every function takes `rules`, a set of rule names turned
OFF one at a time by tests/test_cpu_triang.py.

A KeyFrame is a namespace (tests/triang_cases.py make_kf): n, kp (mvKeysUn) / kp_raw (mvKeys) float32 [n,2],
octave, angle, desc uint8 [n,32], u_right, depth, cos_parallax_stereo, mp_state uint8 [n], the FeatureVector CSR
(node_id, node_begin, feat), Rcw, tcw, Rwc, Ow, fx, fy, cx, cy, invfx, invfy, mb, mbf, scale_factors,
scale_factor, Kinv."""
from __future__ import annotations

import numpy as np

f32 = np.float32
TH_LOW = 50
# slot trace codes of the matcher
NOT_COMMON, HAS_MP, NOT_STEREO, DEN_ZERO, NO_CANDIDATE, MATCHED, ROT_REMOVED = range(7)
# pair status codes (rsc_triang.h TriStatus)
OK, SVD_W0, LOW_PARALLAX, BEHIND1, BEHIND2, REPROJ1, REPROJ2, ZERO_DIST, SCALE = range(9)
RULES = ("th_low_kept", "tie_later", "reject_keeps_best", "stereo_ge0", "epipole_strict", "epipole_test",
         "dsqr_double", "den_zero_return", "vbmatched2_unset", "only_stereo_kf2", "else_if_stereo", "mbf_current",
         "w0_skip", "parallax_double", "raw_keys", "reproj_double", "stereo_reproj_third_term", "scale_test",
         "zero_dist_skip", "depth_le0", "unproject_depth_gate")


def popcount_dist(a, b):
    """ORBmatcher::DescriptorDistance (ORBmatcher.cpp:1492-1508)."""
    return int(np.unpackbits(np.bitwise_xor(a, b)).sum())


def dot3(r, x):
    return f32(f32(f32(r[0] * x[0]) + f32(r[1] * x[1])) + f32(r[2] * x[2]))


def norm3(x):
    return f32(np.sqrt(f32(f32(f32(x[0] * x[0]) + f32(x[1] * x[1])) + f32(x[2] * x[2]))))


def epipole(kf1, kf2):
    """:496-502"""
    R, t, Cw = np.asarray(kf2.Rcw, f32), np.asarray(kf2.tcw, f32), np.asarray(kf1.Ow, f32)
    with np.errstate(all="ignore"):
        C2 = [f32(dot3(R[r], Cw) + t[r]) for r in range(3)]
        invz = f32(f32(1.0) / C2[2])
        ex = f32(f32(f32(f32(kf2.fx) * C2[0]) * invz) + f32(kf2.cx))
        ey = f32(f32(f32(f32(kf2.fy) * C2[1]) * invz) + f32(kf2.cy))
    return ex, ey


def epiline(F, x, y):
    """:546-550"""
    F = np.asarray(F, f32).reshape(3, 3)
    abc = [f32(f32(f32(x * F[0, j]) + f32(y * F[1, j])) + F[2, j]) for j in range(3)]
    den = f32(f32(abc[0] * abc[0]) + f32(abc[1] * abc[1]))
    return abc[0], abc[1], abc[2], den


def rot_bin(a1, a2):
    """:612-617"""
    rot = f32(f32(a1) - f32(a2))
    if rot < 0.0:
        rot = f32(rot + f32(360.0))
    v = float(f32(rot * f32(f32(1.0) / f32(30.0))))
    b = int(np.sign(v) * np.floor(abs(v) + 0.5))  # C round(): halves away from zero
    return 0 if b == 30 else b


def three_maxima(hist):
    """ComputeThreeMaxima (ORBmatcher.cpp:1446-1487) over bin sizes."""
    m1 = m2 = m3 = 0
    i1 = i2 = i3 = -1
    for i, s in enumerate(hist):
        if s > m1:
            m3, m2, m1 = m2, m1, s
            i3, i2, i1 = i2, i1, i
        elif s > m2:
            m3, m2 = m2, s
            i3, i2 = i2, i
        elif s > m3:
            m3, i3 = s, i
    if m2 < f32(f32(0.1) * f32(m1)):
        i2 = i3 = -1
    elif m3 < f32(f32(0.1) * f32(m1)):
        i3 = -1
    return i1, i2, i3


def has_mp(kf, given=None):
    return (np.asarray(kf.mp_state) != 0) if given is None else (np.asarray(given) != 0)


def common_nodes(kf1, kf2):
    """The merge walk of :523-635: (k1, k2) of every node id both FeatureVectors hold, ascending."""
    pos2 = {int(v): k for k, v in enumerate(kf2.node_id)}
    return [(k1, pos2[int(v)]) for k1, v in enumerate(kf1.node_id) if int(v) in pos2]


def candidate_ok(a, b, c, den, ex, ey, st1, st2, x2, y2, sf2, rules=()):
    """:585-597"""
    with np.errstate(all="ignore"):
        if not st1 and not st2 and "epipole_test" not in rules:
            dx, dy = f32(ex - x2), f32(ey - y2)
            d2 = f32(f32(dx * dx) + f32(dy * dy))
            lim = f32(f32(100.0) * sf2)
            if (d2 <= lim) if "epipole_strict" in rules else (d2 < lim):
                return False
        num = f32(f32(f32(a * x2) + f32(b * y2)) + c)
        dsqr = f32(f32(num * num) / den)
        sigma2 = f32(sf2 * sf2)
        if "dsqr_double" in rules:
            return bool(dsqr < f32(f32(3.84) * sigma2))
        return bool(float(dsqr) < 3.84 * float(sigma2))


def is_stereo(u, rules=()):
    return bool(u > 0) if "stereo_ge0" in rules else bool(u >= 0)


def search_for_triangulation(kf1, kf2, F12, only_stereo=False, check_ori=False, has1=None, has2=None, rules=(),
                             all_den_zero=False):
    """:489-669.  Returns matches12 int32 [n1], nmatches, den_zero, den_zero_slot uint8 [n1] (the slot whose den == 0
    ended the call; with all_den_zero every eligible slot with den == 0, the walk going on as if it had not ended:
    what the device reports for the driver) and the per-slot trace (code, winner, bin)."""
    n1 = int(kf1.n)
    ex, ey = epipole(kf1, kf2)
    h1, h2 = has_mp(kf1, has1), has_mp(kf2, has2)
    m12 = np.full(n1, -1, np.int32)
    matched2 = np.zeros(int(kf2.n), bool)
    code = np.full(n1, NOT_COMMON, np.int32)
    win = np.full(n1, -1, np.int32)
    bins = np.full(n1, -1, np.int32)
    dzs = np.zeros(n1, np.uint8)
    rot_hist = [[] for _ in range(30)]
    nmatches, den_zero = 0, 0
    sf = np.asarray(kf2.scale_factors, f32)
    for k1, k2 in common_nodes(kf1, kf2):
        f2 = [int(v) for v in kf2.feat[kf2.node_begin[k2]:kf2.node_begin[k2 + 1]]]
        for idx1 in (int(v) for v in kf1.feat[kf1.node_begin[k1]:kf1.node_begin[k1 + 1]]):
            if h1[idx1]:
                code[idx1] = HAS_MP
                continue
            st1 = is_stereo(kf1.u_right[idx1], rules)
            if only_stereo and not st1:
                code[idx1] = NOT_STEREO
                continue
            a, b, c, den = epiline(F12, f32(kf1.kp[idx1, 0]), f32(kf1.kp[idx1, 1]))
            if den == 0 and "den_zero_return" not in rules:
                code[idx1] = DEN_ZERO
                dzs[idx1] = 1
                den_zero = 1
                if all_den_zero:
                    continue
                return dict(matches12=np.full(n1, -1, np.int32), nmatches=0, den_zero=1, den_zero_slot=dzs, code=code,
                            winner=win, bin=bins)
            best_dist, best = TH_LOW, -1
            for idx2 in f2:
                if matched2[idx2] or h2[idx2]:
                    continue
                st2 = is_stereo(kf2.u_right[idx2], rules)
                if only_stereo and not st2 and "only_stereo_kf2" not in rules:
                    continue
                dist = popcount_dist(kf1.desc[idx1], kf2.desc[idx2])
                if "th_low_kept" in rules and dist >= TH_LOW:
                    continue
                if dist > TH_LOW or (dist >= best_dist if "tie_later" in rules and best >= 0 else dist > best_dist):
                    continue
                ok = candidate_ok(a, b, c, den, ex, ey, st1, st2, f32(kf2.kp[idx2, 0]), f32(kf2.kp[idx2, 1]),
                                  sf[int(kf2.octave[idx2])], rules)
                if ok:
                    best, best_dist = idx2, dist
                elif "reject_keeps_best" in rules:
                    best_dist = dist
            if best >= 0:
                m12[idx1] = best
                nmatches += 1
                code[idx1], win[idx1] = MATCHED, best
                if "vbmatched2_unset" in rules:
                    matched2[best] = True
                if check_ori:
                    bins[idx1] = rot_bin(kf1.angle[idx1], kf2.angle[best])
                    rot_hist[bins[idx1]].append(idx1)
            else:
                code[idx1] = NO_CANDIDATE
    if den_zero:  # all_den_zero: the call's result is still the empty one
        return dict(matches12=np.full(n1, -1, np.int32), nmatches=0, den_zero=1, den_zero_slot=dzs, code=code,
                    winner=win, bin=bins, spec_matches12=m12)
    if check_ori:
        keep = three_maxima([len(h) for h in rot_hist])
        for i in range(30):
            if i in keep:
                continue
            for idx1 in rot_hist[i]:
                m12[idx1] = -1
                code[idx1] = ROT_REMOVED
                nmatches -= 1
    return dict(matches12=m12, nmatches=nmatches, den_zero=0, den_zero_slot=dzs, code=code, winner=win, bin=bins,
                spec_matches12=m12)


def matched_pairs(m12):
    """vMatchedPairs (:658-666)."""
    return [(int(i), int(v)) for i, v in enumerate(m12) if v >= 0]


# ---- the pair geometry ------------------------------------------------------------------------------------------

def jacobi_2x2(m00, m01, m10, m11):
    """real_2x2_jacobi_svd (Eigen/src/SVD/JacobiSVD.h) in float."""
    tiny = f32(np.finfo(np.float32).tiny)
    one = f32(1.0)
    with np.errstate(all="ignore"):
        t = f32(m00 + m11)
        d = f32(m10 - m01)
        if abs(d) < tiny:
            s1, c1 = f32(0.0), one
        else:
            u = f32(t / d)
            tmp = f32(np.sqrt(f32(one + f32(u * u))))
            s1, c1 = f32(one / tmp), f32(u / tmp)
        if not (c1 == 1.0 and s1 == 0.0):
            x0, y0, x1, y1 = m00, m10, m01, m11
            m00, m10 = f32(f32(c1 * x0) + f32(s1 * y0)), f32(f32(-s1 * x0) + f32(c1 * y0))
            m01, m11 = f32(f32(c1 * x1) + f32(s1 * y1)), f32(f32(-s1 * x1) + f32(c1 * y1))
        deno = f32(f32(2.0) * abs(m01))
        if deno < tiny:
            cr, sr = one, f32(0.0)
        else:
            tau = f32(f32(m00 - m11) / deno)
            w = f32(np.sqrt(f32(f32(tau * tau) + one)))
            tt = f32(one / (f32(tau + w) if tau > 0 else f32(tau - w)))
            sign_t = one if tt > 0 else f32(-1.0)
            nn = f32(one / f32(np.sqrt(f32(f32(tt * tt) + one))))
            sr = f32(f32(f32(-sign_t * f32(m01 / abs(m01))) * abs(tt)) * nn)
            cr = nn
        cl = f32(f32(c1 * cr) - f32(s1 * f32(-sr)))
        sl = f32(f32(c1 * f32(-sr)) + f32(s1 * cr))
    return cl, sl, cr, sr


def svd_last_v(A):
    """JacobiSVD<Matrix4f>(A, ComputeFullV).matrixV().rightCols<1>() restated (rsc_triang.h tri_svd_last_v)."""
    A = np.asarray(A, f32)
    eps2 = f32(f32(2.0) * f32(np.finfo(np.float32).eps))
    tiny = f32(np.finfo(np.float32).tiny)
    scale = abs(A[0, 0])
    for c in range(4):
        for r in range(4):
            if abs(A[r, c]) > scale:
                scale = abs(A[r, c])
    if scale == 0:
        scale = f32(1.0)
    with np.errstate(all="ignore"):
        W = (A / scale).astype(f32)
        V = np.eye(4, dtype=f32)
        max_diag = max(abs(W[i, i]) for i in range(4))
        if not max_diag == max_diag:  # max() over NaNs: follow the kernel's `>` updates from W[0][0]
            max_diag = abs(W[0, 0])
            for i in range(1, 4):
                if abs(W[i, i]) > max_diag:
                    max_diag = abs(W[i, i])
        finished = False
        while not finished:
            finished = True
            for p in range(1, 4):
                for q in range(p):
                    pt = f32(eps2 * max_diag)
                    th = pt if tiny < pt else tiny
                    if abs(W[p, q]) > th or abs(W[q, p]) > th:
                        finished = False
                        cl, sl, cr, sr = jacobi_2x2(W[p, p], W[p, q], W[q, p], W[q, q])
                        if not (cl == 1.0 and sl == 0.0):
                            xp, xq = W[p].copy(), W[q].copy()
                            W[p] = (cl * xp).astype(f32) + (sl * xq).astype(f32)
                            W[q] = (-sl * xp).astype(f32) + (cl * xq).astype(f32)
                        if not (cr == 1.0 and sr == 0.0):
                            for M in (W, V):
                                xp, xq = M[:, p].copy(), M[:, q].copy()
                                M[:, p] = (cr * xp).astype(f32) - (sr * xq).astype(f32)
                                M[:, q] = (sr * xp).astype(f32) + (cr * xq).astype(f32)
                        a, b = abs(W[p, p]), abs(W[q, q])
                        mm = b if a < b else a
                        max_diag = mm if max_diag < mm else max_diag
        sv = [f32(abs(W[i, i]) * scale) for i in range(4)]
    for i in range(4):
        pos, mv = 0, sv[i]
        for j in range(1, 4 - i):
            if sv[i + j] > mv:
                mv, pos = sv[i + j], j
        if mv == 0:
            break
        if pos:
            sv[i], sv[i + pos] = sv[i + pos], sv[i]
            V[:, [i, i + pos]] = V[:, [i + pos, i]]
    return V[:, 3].copy()


def triangulation_matrix(kf1, kf2, xn1, xn2):
    """A of :298-301."""
    A = np.zeros((4, 4), f32)
    for row, (kf, xn) in enumerate(((kf1, xn1), (kf2, xn2))):
        T = np.concatenate([np.asarray(kf.Rcw, f32), np.asarray(kf.tcw, f32).reshape(3, 1)], 1)
        for c in range(4):
            A[2 * row, c] = f32(f32(xn[0] * T[2, c]) - T[0, c])
            A[2 * row + 1, c] = f32(f32(xn[1] * T[2, c]) - T[1, c])
    return A


def unproject_stereo(kf, i, rules=()):
    """KeyFrame::UnprojectStereo (KeyFrame.cpp:606-622)."""
    z = f32(kf.depth[i])
    if z > 0 or "unproject_depth_gate" in rules:
        src = kf.kp if "raw_keys" in rules else kf.kp_raw
        u, v = f32(src[i, 0]), f32(src[i, 1])
        xc = [f32(f32(f32(u - f32(kf.cx)) * z) * f32(kf.invfx)), f32(f32(f32(v - f32(kf.cy)) * z) * f32(kf.invfy)), z]
        R, O = np.asarray(kf.Rwc, f32), np.asarray(kf.Ow, f32)
        return np.array([f32(dot3(R[r], xc) + O[r]) for r in range(3)], f32)
    return np.zeros(3, f32)


def reproj_ok(kf, x3D, z, idx, ur, stereo, mbf, rules=()):
    """:339-389"""
    R, t = np.asarray(kf.Rcw, f32), np.asarray(kf.tcw, f32)
    sfo = f32(np.asarray(kf.scale_factors, f32)[int(kf.octave[idx])])
    sigma2 = f32(sfo * sfo)
    with np.errstate(all="ignore"):
        x = f32(dot3(R[0], x3D) + t[0])
        y = f32(dot3(R[1], x3D) + t[1])
        invz = f32(np.float64(1.0) / np.float64(z))
        u = f32(f32(f32(f32(kf.fx) * x) * invz) + f32(kf.cx))
        v = f32(f32(f32(f32(kf.fy) * y) * invz) + f32(kf.cy))
        ex_, ey_ = f32(u - f32(kf.kp[idx, 0])), f32(v - f32(kf.kp[idx, 1]))
        e = f32(f32(ex_ * ex_) + f32(ey_ * ey_))
        chi = 5.991
        if stereo:
            chi = 7.8
            if "stereo_reproj_third_term" not in rules:
                er = f32(f32(u - f32(f32(mbf) * invz)) - f32(ur))
                e = f32(e + f32(er * er))
        if "reproj_double" in rules:
            return not bool(e > f32(f32(chi) * sigma2))
        return not (float(e) > chi * float(sigma2))


def triangulate_pair(kf1, kf2, idx1, idx2, rules=()):
    """LocalMapping.cpp:262-407 for one pair.  Returns (status, x3D float32 [3], trace dict)."""
    x3D = np.zeros(3, f32)
    ur1, ur2 = f32(kf1.u_right[idx1]), f32(kf2.u_right[idx2])
    st1, st2 = bool(ur1 >= 0), bool(ur2 >= 0)
    xn1 = [f32(f32(f32(kf1.kp[idx1, 0]) - f32(kf1.cx)) * f32(kf1.invfx)),
           f32(f32(f32(kf1.kp[idx1, 1]) - f32(kf1.cy)) * f32(kf1.invfy)), f32(1.0)]
    xn2 = [f32(f32(f32(kf2.kp[idx2, 0]) - f32(kf2.cx)) * f32(kf2.invfx)),
           f32(f32(f32(kf2.kp[idx2, 1]) - f32(kf2.cy)) * f32(kf2.invfy)), f32(1.0)]
    R1, R2 = np.asarray(kf1.Rcw, f32), np.asarray(kf2.Rcw, f32)
    t1, t2 = np.asarray(kf1.tcw, f32), np.asarray(kf2.tcw, f32)
    with np.errstate(all="ignore"):
        ray1 = [dot3(R1[:, r], xn1) for r in range(3)]  # Rwc = Rcw.transpose() (:205)
        ray2 = [dot3(R2[:, r], xn2) for r in range(3)]
        cos_rays = f32(dot3(ray1, ray2) / f32(norm3(ray1) * norm3(ray2)))
        cs = f32(cos_rays + f32(1.0))
        cs1 = cs2 = cs
        if st1:
            cs1 = f32(kf1.cos_parallax_stereo[idx1])
        elif st2:
            cs2 = f32(kf2.cos_parallax_stereo[idx2])
        if "else_if_stereo" in rules and st1 and st2:
            cs2 = f32(kf2.cos_parallax_stereo[idx2])
        cs = cs2 if cs2 < cs1 else cs1
        low = bool(cos_rays < f32(0.9998)) if "parallax_double" in rules else (float(cos_rays) < 0.9998)
        tr = dict(cos_rays=cos_rays, branch="skip")
        if cos_rays < cs and cos_rays > 0 and (st1 or st2 or low):
            tr["branch"] = "svd"
            A = triangulation_matrix(kf1, kf2, xn1, xn2)
            tr["A"] = A
            temp = svd_last_v(A)
            if temp[3] == 0 and "w0_skip" not in rules:
                return SVD_W0, x3D, tr
            x3D = np.array([f32(temp[0] / temp[3]), f32(temp[1] / temp[3]), f32(temp[2] / temp[3])], f32)
        elif st1 and cs1 < cs2:
            tr["branch"] = "stereo1"
            x3D = unproject_stereo(kf1, idx1, rules)
        elif st2 and cs2 < cs1:
            tr["branch"] = "stereo2"
            x3D = unproject_stereo(kf2, idx2, rules)
        else:
            return LOW_PARALLAX, x3D, tr
        z1 = f32(dot3(R1[2], x3D) + t1[2])
        if (z1 < 0) if "depth_le0" in rules else (z1 <= 0):
            return BEHIND1, x3D, tr
        z2 = f32(dot3(R2[2], x3D) + t2[2])
        if (z2 < 0) if "depth_le0" in rules else (z2 <= 0):
            return BEHIND2, x3D, tr
        if not reproj_ok(kf1, x3D, z1, idx1, ur1, st1, kf1.mbf, rules):
            return REPROJ1, x3D, tr
        # :382 reads mpCurrentKeyFrame->mbf for KeyFrame 2's right-image error
        if not reproj_ok(kf2, x3D, z2, idx2, ur2, st2, kf2.mbf if "mbf_current" in rules else kf1.mbf, rules):
            return REPROJ2, x3D, tr
        O1, O2 = np.asarray(kf1.Ow, f32), np.asarray(kf2.Ow, f32)
        d1 = norm3([f32(x3D[i] - O1[i]) for i in range(3)])
        d2 = norm3([f32(x3D[i] - O2[i]) for i in range(3)])
        if (d1 == 0 or d2 == 0) and "zero_dist_skip" not in rules:
            return ZERO_DIST, x3D, tr
        ratio_factor = f32(f32(1.5) * f32(kf1.scale_factor))
        ratio_dist = f32(d2 / d1)
        s1 = f32(np.asarray(kf1.scale_factors, f32)[int(kf1.octave[idx1])])
        s2 = f32(np.asarray(kf2.scale_factors, f32)[int(kf2.octave[idx2])])
        ratio_oct = f32(s1 / s2)
        if "scale_test" not in rules and (f32(ratio_dist * ratio_factor) < ratio_oct or
                                          ratio_dist > f32(ratio_oct * ratio_factor)):
            return SCALE, x3D, tr
    return OK, x3D, tr


# ---- the driver -------------------------------------------------------------------------------------------------

def mul33(A, B):
    A, B = np.asarray(A, f32).reshape(3, 3), np.asarray(B, f32).reshape(3, 3)
    return np.array([[dot3(A[r], B[:, c]) for c in range(3)] for r in range(3)], f32)


def compute_f12(kf1, kf2):
    """LocalMapping::ComputeF12 (:512-531): T12 = T1w * T2wi, F12 = K1inv^T * t12x * R12 * K2inv, left to right."""
    R1, t1 = np.asarray(kf1.Rcw, f32), np.asarray(kf1.tcw, f32)
    R2i, t2i = np.asarray(kf2.Rwc, f32), np.asarray(kf2.Ow, f32)
    with np.errstate(all="ignore"):
        R12 = mul33(R1, R2i)
        t12 = [f32(dot3(R1[r], t2i) + t1[r]) for r in range(3)]
        z = f32(0.0)
        t12x = np.array([[z, -t12[2], t12[1]], [t12[2], z, -t12[0]], [-t12[1], t12[0], z]], f32)
        return mul33(mul33(mul33(np.asarray(kf1.Kinv, f32).reshape(3, 3).T, t12x), R12), kf2.Kinv)


def baseline_short(kf1, kf2):
    """:232-236"""
    O1, O2 = np.asarray(kf1.Ow, f32), np.asarray(kf2.Ow, f32)
    return bool(norm3([f32(O2[i] - O1[i]) for i in range(3)]) < f32(kf2.mb))


def _empty(n):
    return dict(new_neighbour=np.full(n, -1, np.int32), new_idx2=np.full(n, -1, np.int32),
                new_pos=np.zeros((n, 3), f32), nnew=0, order=[])


def create_new_map_points(cur, neighbours):
    """The literal neighbour loop of :224-428: slots are filled as it goes.  `order`: (neighbour, idx1) as created."""
    out = _empty(int(cur.n))
    filled = (np.asarray(cur.mp_state) != 0).astype(np.uint8)
    voided = []
    for i, kf2 in enumerate(neighbours):
        if baseline_short(cur, kf2):
            continue
        F12 = compute_f12(cur, kf2)
        r = search_for_triangulation(cur, kf2, F12, False, False, has1=filled)
        if r["den_zero"]:
            voided.append(i)
        for idx1, idx2 in matched_pairs(r["matches12"]):
            st, x3D, _ = triangulate_pair(cur, kf2, idx1, idx2)
            if st != OK:
                continue
            out["new_neighbour"][idx1], out["new_idx2"][idx1], out["new_pos"][idx1] = i, idx2, x3D
            filled[idx1] = 1  # AddMapPoint (:415)
            out["nnew"] += 1
            out["order"].append((i, idx1))
    out["voided"] = voided
    return out


def create_new_map_points_speculative(cur, neighbours):
    """rsc_create_new_map_points_many's shape: every neighbour matched and triangulated from the INITIAL slots, then
    the neighbour order replayed."""
    out = _empty(int(cur.n))
    spec = []
    for i, kf2 in enumerate(neighbours):
        if baseline_short(cur, kf2):
            continue
        r = search_for_triangulation(cur, kf2, compute_f12(cur, kf2), False, False, all_den_zero=True)
        prs = matched_pairs(r["spec_matches12"])
        spec.append((i, r["den_zero_slot"], prs, [triangulate_pair(cur, kf2, a, b)[:2] for a, b in prs]))
    filled = (np.asarray(cur.mp_state) != 0).astype(np.uint8)
    for i, dzs, prs, tri in spec:
        if np.any((dzs != 0) & (filled == 0)):
            continue
        for (idx1, idx2), (st, x3D) in zip(prs, tri):
            if filled[idx1] or st != OK:
                continue
            out["new_neighbour"][idx1], out["new_idx2"][idx1], out["new_pos"][idx1] = i, idx2, x3D
            filled[idx1] = 1
            out["nnew"] += 1
            out["order"].append((i, idx1))
    return out
