"""ctypes binding of librsc.so (include/rsc.h) with the reference's solver API.

``PnPSolver`` / ``Sim3Solver`` mirror ORB_SLAM_CUSTOM::PnPsolver / Sim3Solver
(include/PnPsolver.hpp:24-31, include/Sim3Solver.hpp:21-30): same constructor inputs (already
reduced to plain arrays), ``set_ransac_parameters`` / ``iterate`` / ``find`` with the same argument
meaning and results.  Every call runs on the MI355X; there is no CPU fallback — if librsc.so is
missing or no HIP device is present the calls raise ``RuntimeError``.
"""
from __future__ import annotations

import ctypes as C
import os
import numpy as np

PKG_DIR = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# RSC_LIBRSC: another build of the same library (A/B kernel comparisons in tools/); the default is
# the in-tree build.
LIB_PATH = os.environ.get("RSC_LIBRSC") or os.path.join(PKG_DIR, "lib", "librsc.so")

RSC_OK = 0

_lib = None

f32p = np.ctypeslib.ndpointer(dtype=np.float32, flags="C_CONTIGUOUS")
i32p = np.ctypeslib.ndpointer(dtype=np.int32, flags="C_CONTIGUOUS")
u64p = np.ctypeslib.ndpointer(dtype=np.uint64, flags="C_CONTIGUOUS")
u8p = np.ctypeslib.ndpointer(dtype=np.uint8, flags="C_CONTIGUOUS")

# Every symbol declared in include/rsc.h (checked by tests/test_cpu_abi.py).
EXPORTED = [
    "rsc_version", "rsc_status_string", "rsc_context_create", "rsc_context_destroy", "rsc_context_set_stream",
    "rsc_context_synchronize", "rsc_context_last_timing", "rsc_context_last_kernel_timing", "rsc_diag_host_timing", "rsc_context_enable_timing", "rsc_selftest_math",
    "rsc_context_set_eig_rows", "rsc_context_set_eig_split", "rsc_context_set_sim3opt_helpers",
    "rsc_context_set_round_args", "rsc_context_set_scan_bound", "rsc_pnp_last_counts_raw", "rsc_diag_round_paths",
    "rsc_pnp_create", "rsc_pnp_destroy", "rsc_pnp_set_ransac_parameters", "rsc_pnp_iterate", "rsc_pnp_find",
    "rsc_pnp_last_inliers",
    "rsc_pnp_iterate_many", "rsc_pnp_reset", "rsc_pnp_get_state", "rsc_pnp_last_samples", "rsc_pnp_last_hypotheses",
    "rsc_sim3_last_hypotheses", "rsc_mlpnp_last_counts",
    "rsc_sim3_create", "rsc_sim3_destroy", "rsc_sim3_set_ransac_parameters", "rsc_sim3_iterate", "rsc_sim3_find",
    "rsc_sim3_iterate_many", "rsc_sim3_reset", "rsc_sim3_get_state", "rsc_sim3_prepared", "rsc_rand_stream",
    "rsc_pnp_reset_many", "rsc_pnp_set_ransac_parameters_many", "rsc_sim3_reset_many",
    "rsc_sim3_set_ransac_parameters_many",
    "rsc_mlpnp_create", "rsc_mlpnp_destroy", "rsc_mlpnp_set_covariances", "rsc_mlpnp_set_ransac_parameters",
    "rsc_mlpnp_set_ransac_parameters_many", "rsc_mlpnp_iterate", "rsc_mlpnp_iterate_many", "rsc_mlpnp_reset",
    "rsc_mlpnp_reset_many", "rsc_mlpnp_get_state", "rsc_mlpnp_last_poses", "rsc_mlpnp_last_samples",
    "rsc_reloc_events", "rsc_loop_events", "rsc_pose_optimization_many",
    "rsc_bow_create", "rsc_bow_destroy", "rsc_bow_set_valid", "rsc_search_by_bow_frame_many",
    "rsc_search_by_bow_kf_many", "rsc_diag_bow_phase_stamps", "rsc_diag_refine_phase_stamps", "rsc_diag_solve_phase_stamps", "rsc_diag_poseopt_phases", "rsc_diag_sim3opt_phases", "rsc_diag_kfdb_stamps",
    "rsc_search_by_sim3_many", "rsc_diag_sim3match_directions", "rsc_kfview_create", "rsc_kfview_destroy",
    "rsc_optimize_sim3_many",
    "rsc_kfdb_create", "rsc_kfdb_destroy", "rsc_kfdb_add", "rsc_kfdb_erase", "rsc_kfdb_release", "rsc_kfdb_clear",
    "rsc_kfdb_set_covisibility", "rsc_kfdb_set_covisibility_many", "rsc_kfdb_detect_relocalization", "rsc_kfdb_detect_loop", "rsc_kfdb_state",
    "rsc_stream_create", "rsc_stream_destroy", "rsc_stream_skip", "rsc_stream_position", "rsc_stream_peek",
    "rsc_pnp_bind_stream", "rsc_sim3_bind_stream", "rsc_mlpnp_bind_stream", "rsc_reloc_events_shared",
    "rsc_loop_events_shared", "rsc_reloc_events_gated", "rsc_loop_events_gated",
    "rsc_diag_mlpnp_phase_stamps",
    "rsc_frameview_create", "rsc_frameview_destroy", "rsc_kfview_set_angles", "rsc_search_by_projection_many",
    "rsc_reloc_refine_many", "rsc_reloc_events_refined",
    "rsc_mpview_create", "rsc_mpview_destroy", "rsc_search_by_projection_kf_many", "rsc_fuse_sim3_many",
    "rsc_loop_verify_many",
    "rsc_voc_create", "rsc_voc_destroy", "rsc_voc_size", "rsc_voc_info", "rsc_voc_transform_many",
    "rsc_voc_last_kernel_timing", "rsc_bow_create_transformed",
    "rsc_frameview_set_stereo", "rsc_search_local_points_many", "rsc_search_by_projection_points_many",
    "rsc_lastframe_create", "rsc_lastframe_destroy", "rsc_search_by_projection_last_many",
    "rsc_track_motion_model_many",
    "rsc_kfview_set_triangulation", "rsc_search_for_triangulation_many", "rsc_triangulate_pairs_many",
    "rsc_create_new_map_points_many", "rsc_fuse_kf_many",
    "rsc_update_map_points_many", "rsc_mpview_download",
    "rsc_compute_stereo_matches_many",
    "rsc_diag_fill_staging",
    "rsc_local_bundle_adjustment_many", "rsc_diag_localba_stages",
]

# include/rsc.h RSC_GATE_*
GATE_NONE, GATE_MATCH, GATE_HANDOFF = 0, 1, 2


class EventResult(C.Structure):
    _fields_ = [("winner", C.c_int32), ("round", C.c_int32), ("hypothesis", C.c_int32), ("n_inliers", C.c_int32)]


class RelocFrame(C.Structure):
    _fields_ = [("u_right", C.c_void_p), ("bf", C.c_float)]


class RelocGateResult(C.Structure):
    _fields_ = [("status", C.c_int32), ("winner", C.c_int32), ("round", C.c_int32), ("hypothesis", C.c_int32),
                ("n_inliers", C.c_int32), ("n_good", C.c_int32), ("rejected", C.c_int32), ("gates", C.c_int32),
                ("Tcw", C.c_float * 16)]


class RelocRefineResult(C.Structure):
    """rsc_reloc_refine_result (include/rsc.h)."""
    _fields_ = [("n_good", C.c_int32), ("n_additional", C.c_int32 * 2), ("pose_opts", C.c_int32),
                ("Tcw", C.c_float * 16)]


class RelocCandidate(C.Structure):
    _fields_ = [("kf", C.c_void_p), ("matches", C.c_void_p)]


class RelocRefinedResult(C.Structure):
    """rsc_reloc_refined_result (include/rsc.h)."""
    _fields_ = [("status", C.c_int32), ("winner", C.c_int32), ("round", C.c_int32), ("hypothesis", C.c_int32),
                ("n_inliers", C.c_int32), ("n_good", C.c_int32), ("rejected", C.c_int32), ("gates", C.c_int32),
                ("n_good_first", C.c_int32), ("n_additional", C.c_int32 * 2), ("chains", C.c_int32),
                ("Tcw", C.c_float * 16)]


class FrameFeatures(C.Structure):
    """rsc_frame_features (include/rsc.h)."""
    _fields_ = [("n", C.c_int32), ("kp", C.c_void_p), ("octave", C.c_void_p), ("angle", C.c_void_p),
                ("desc", C.c_void_p), ("cell_begin", C.c_void_p), ("cell_feat", C.c_void_p), ("min_x", C.c_float),
                ("max_x", C.c_float), ("min_y", C.c_float), ("max_y", C.c_float), ("grid_w_inv", C.c_float),
                ("grid_h_inv", C.c_float), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float),
                ("cy", C.c_float), ("scale_factors", C.c_void_p), ("n_levels", C.c_int32),
                ("log_scale_factor", C.c_float)]


class LoopCandidate(C.Structure):
    _fields_ = [("kf1", C.c_void_p), ("kf2", C.c_void_p), ("matches12", C.c_void_p)]


class LoopGateResult(C.Structure):
    _fields_ = [("status", C.c_int32), ("winner", C.c_int32), ("round", C.c_int32), ("hypothesis", C.c_int32),
                ("n_inliers", C.c_int32), ("n_found", C.c_int32), ("n_opt_inliers", C.c_int32),
                ("rejected", C.c_int32), ("S", C.c_double * 8)]


class PnPProblem(C.Structure):
    _fields_ = [("n", C.c_int32), ("n_points", C.c_int32), ("p2d", C.c_void_p), ("p3dw", C.c_void_p),
                ("sigma2", C.c_void_p), ("kp_index", C.c_void_p), ("fx", C.c_float), ("fy", C.c_float),
                ("cx", C.c_float), ("cy", C.c_float)]


class PnPResult(C.Structure):
    _fields_ = [("ok", C.c_int32), ("no_more", C.c_int32), ("n_inliers", C.c_int32), ("iterations", C.c_int32),
                ("T", C.c_float * 16)]


class Sim3Input(C.Structure):
    _fields_ = [("n1", C.c_int32), ("valid", C.c_void_p), ("Xw1", C.c_void_p), ("Xw2", C.c_void_p),
                ("sigma2_1", C.c_void_p), ("sigma2_2", C.c_void_p), ("R1", C.c_float * 9), ("t1", C.c_float * 3),
                ("R2", C.c_float * 9), ("t2", C.c_float * 3), ("K1", C.c_float * 4), ("K2", C.c_float * 4)]


class Sim3Result(C.Structure):
    _fields_ = [("ok", C.c_int32), ("no_more", C.c_int32), ("n_inliers", C.c_int32), ("iterations", C.c_int32),
                ("R", C.c_float * 9), ("t", C.c_float * 3)]


class PoseOptProblem(C.Structure):
    _fields_ = [("n", C.c_int32), ("has_mp", C.c_void_p), ("uv", C.c_void_p), ("Xw", C.c_void_p),
                ("inv_sigma2", C.c_void_p), ("u_right", C.c_void_p), ("fx", C.c_float), ("fy", C.c_float),
                ("cx", C.c_float), ("cy", C.c_float), ("Tcw", C.c_float * 16), ("bf", C.c_float)]


class Sim3OptProblem(C.Structure):
    _fields_ = [("n", C.c_int32), ("valid", C.c_void_p), ("X1w", C.c_void_p), ("X2w", C.c_void_p),
                ("uv1", C.c_void_p), ("uv2", C.c_void_p), ("inv1", C.c_void_p), ("inv2", C.c_void_p),
                ("R1w", C.c_float * 9), ("t1w", C.c_float * 3), ("R2w", C.c_float * 9), ("t2w", C.c_float * 3),
                ("K1", C.c_float * 4), ("K2", C.c_float * 4), ("S", C.c_double * 8), ("th2", C.c_float)]


class Sim3OptResult(C.Structure):
    _fields_ = [("n_inliers", C.c_int32), ("n_correspondences", C.c_int32), ("n_bad", C.c_int32),
                ("lm_iterations", C.c_int32), ("lm_trials", C.c_int32), ("S", C.c_double * 8)]


class BowFeatures(C.Structure):
    _fields_ = [("n", C.c_int32), ("desc", C.c_void_p), ("angle", C.c_void_p), ("valid", C.c_void_p),
                ("n_nodes", C.c_int32), ("node_id", C.c_void_p), ("node_begin", C.c_void_p), ("feat", C.c_void_p)]


class VocabularyNodes(C.Structure):
    _fields_ = [("k", C.c_int32), ("L", C.c_int32), ("scoring", C.c_int32), ("weighting", C.c_int32),
                ("n_nodes", C.c_int32), ("parent", C.c_void_p), ("is_leaf", C.c_void_p), ("desc", C.c_void_p),
                ("weight", C.c_void_p), ("lds_budget_bytes", C.c_int32)]


class VocOutput(C.Structure):
    _fields_ = [("n_words", C.c_int32), ("word_id", C.c_void_p), ("word_value", C.c_void_p),
                ("n_nodes", C.c_int32), ("node_id", C.c_void_p), ("node_begin", C.c_void_p), ("feat", C.c_void_p),
                ("feature_word", C.c_void_p), ("feature_node", C.c_void_p), ("feature_stopped", C.c_void_p)]


class Sim3KFStruct(C.Structure):
    """rsc_sim3_kf (include/rsc.h)."""
    _fields_ = [("n", C.c_int32), ("kp", C.c_void_p), ("octave", C.c_void_p), ("desc", C.c_void_p),
                ("cell_begin", C.c_void_p), ("cell_feat", C.c_void_p), ("min_x", C.c_float), ("max_x", C.c_float),
                ("min_y", C.c_float), ("max_y", C.c_float), ("grid_w_inv", C.c_float), ("grid_h_inv", C.c_float),
                ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
                ("scale_factors", C.c_void_p), ("n_levels", C.c_int32), ("log_scale_factor", C.c_float),
                ("Rcw", C.c_float * 9), ("tcw", C.c_float * 3), ("mp_state", C.c_void_p), ("mp_pos", C.c_void_p),
                ("mp_dmax", C.c_void_p), ("mp_dmin", C.c_void_p), ("mp_desc", C.c_void_p)]


class KFTriangulation(C.Structure):
    """rsc_kf_triangulation (include/rsc.h)."""
    _fields_ = [("u_right", C.c_void_p), ("depth", C.c_void_p), ("kp_raw", C.c_void_p),
                ("cos_parallax_stereo", C.c_void_p), ("mb", C.c_float), ("mbf", C.c_float), ("invfx", C.c_float),
                ("invfy", C.c_float), ("scale_factor", C.c_float), ("Rwc", C.c_float * 9), ("Ow", C.c_float * 3),
                ("Kinv", C.c_float * 9)]


def sim3_kf_struct(kf):
    """(ctypes rsc_sim3_kf, keep-alive arrays) for a rsc.synth.Sim3KF-like object."""
    from rsc import synth
    sf, log_sf, gw_inv, gh_inv = synth.kf_geometry(kf)  # the KeyFrame's own, else the synth constants
    keep = [np.ascontiguousarray(kf.kp, np.float32), np.ascontiguousarray(kf.octave, np.int32),
            np.ascontiguousarray(kf.desc, np.uint8), np.ascontiguousarray(kf.cell_begin, np.int32),
            np.ascontiguousarray(kf.cell_feat, np.int32), sf,
            np.ascontiguousarray(kf.mp_state, np.uint8), np.ascontiguousarray(kf.mp_pos, np.float32),
            np.ascontiguousarray(kf.mp_dmax, np.float32), np.ascontiguousarray(kf.mp_dmin, np.float32),
            np.ascontiguousarray(kf.mp_desc, np.uint8)]
    if keep[4].size == 0:
        keep[4] = np.zeros(1, np.int32)
    k = Sim3KFStruct()
    k.n = int(kf.n)
    (k.kp, k.octave, k.desc, k.cell_begin, k.cell_feat, k.scale_factors, k.mp_state, k.mp_pos, k.mp_dmax,
     k.mp_dmin, k.mp_desc) = (a.ctypes.data for a in keep)
    k.min_x, k.max_x, k.min_y, k.max_y = kf.min_x, kf.max_x, kf.min_y, kf.max_y
    k.grid_w_inv, k.grid_h_inv = float(gw_inv), float(gh_inv)
    k.fx, k.fy, k.cx, k.cy = kf.fx, kf.fy, kf.cx, kf.cy
    k.n_levels = len(keep[5])
    k.log_scale_factor = float(log_sf)
    k.Rcw[:] = [float(v) for v in np.asarray(kf.Rcw, np.float32).reshape(9)]
    k.tcw[:] = [float(v) for v in np.asarray(kf.tcw, np.float32).reshape(3)]
    return k, keep


class KFView:
    """A KeyFrame's SearchBySim3 inputs resident in HBM (rsc_kfview_create)."""

    def __init__(self, ctx: Context, kf):
        self.ctx, self.n = ctx, int(kf.n)
        k, keep = sim3_kf_struct(kf)
        h = C.c_void_p()
        _check(load_library().rsc_kfview_create(ctx.h, C.byref(k), C.byref(h)), "rsc_kfview_create")
        self.h = h

    def set_angles(self, angle):
        """mvKeysUn[i].angle of the KeyFrame (the rotation check of SearchByProjection reads them)."""
        a = np.ascontiguousarray(angle, np.float32)
        if a.size != self.n:
            raise ValueError(f"{self.n} angles expected, got {a.size}")
        _check(load_library().rsc_kfview_set_angles(self.h, a if a.size else np.zeros(1, np.float32)),
               "rsc_kfview_set_angles")

    def set_triangulation(self, tri):
        """What CreateNewMapPoints reads and the view lacks (rsc_kfview_set_triangulation): an object with u_right,
        depth, cos_parallax_stereo float32 [n], kp_raw float32 [n,2], mb, mbf, invfx, invfy, scale_factor, Rwc [3,3],
        Ow [3] (Twc as KeyFrame::SetPose stores it) and Kinv [3,3] (KeyFrame::mKinv)."""
        pad = lambda a, k: (np.ascontiguousarray(a, np.float32).reshape(-1) if self.n else np.zeros(k, np.float32))
        keep = [pad(tri.u_right, 1), pad(tri.depth, 1), pad(tri.kp_raw, 2), pad(tri.cos_parallax_stereo, 1)]
        assert keep[0].size == max(self.n, 1) and keep[2].size == 2 * max(self.n, 1)
        t = KFTriangulation()
        t.u_right, t.depth, t.kp_raw, t.cos_parallax_stereo = (a.ctypes.data for a in keep)
        t.mb, t.mbf, t.invfx, t.invfy = float(tri.mb), float(tri.mbf), float(tri.invfx), float(tri.invfy)
        t.scale_factor = float(tri.scale_factor)
        t.Rwc[:] = [float(v) for v in np.asarray(tri.Rwc, np.float32).reshape(9)]
        t.Ow[:] = [float(v) for v in np.asarray(tri.Ow, np.float32).reshape(3)]
        t.Kinv[:] = [float(v) for v in np.asarray(tri.Kinv, np.float32).reshape(9)]
        _check(load_library().rsc_kfview_set_triangulation(self.h, C.byref(t)), "rsc_kfview_set_triangulation")

    def close(self):
        if getattr(self, "h", None):
            load_library().rsc_kfview_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()


def frame_features_struct(fr):
    """(ctypes rsc_frame_features, keep-alive arrays) for a rsc.synth.ProjFrame-like object."""
    from rsc import synth
    keep = [np.ascontiguousarray(fr.kp, np.float32), np.ascontiguousarray(fr.octave, np.int32),
            np.ascontiguousarray(fr.angle, np.float32), np.ascontiguousarray(fr.desc, np.uint8),
            np.ascontiguousarray(fr.cell_begin, np.int32), np.ascontiguousarray(fr.cell_feat, np.int32),
            synth.scale_factors()]
    if keep[5].size == 0:
        keep[5] = np.zeros(1, np.int32)
    k = FrameFeatures()
    k.n = int(fr.n)
    k.kp, k.octave, k.angle, k.desc, k.cell_begin, k.cell_feat, k.scale_factors = (a.ctypes.data for a in keep)
    k.min_x, k.max_x, k.min_y, k.max_y = fr.min_x, fr.max_x, fr.min_y, fr.max_y
    k.grid_w_inv, k.grid_h_inv = float(synth.GRID_W_INV), float(synth.GRID_H_INV)
    k.fx, k.fy, k.cx, k.cy = fr.fx, fr.fy, fr.cx, fr.cy
    k.n_levels = len(keep[6])
    k.log_scale_factor = float(synth.LOG_SCALE_FACTOR)
    return k, keep


class FrameView:
    """The current Frame as SearchByProjection reads it, resident in HBM (rsc_frameview_create)."""

    def __init__(self, ctx: Context, fr):
        self.ctx, self.n = ctx, int(fr.n)
        k, keep = frame_features_struct(fr)
        h = C.c_void_p()
        _check(load_library().rsc_frameview_create(ctx.h, C.byref(k), C.byref(h)), "rsc_frameview_create")
        self.h = h

    def set_stereo(self, u_right, mbf: float):
        """The Frame's mvuRight (float32 [n], negative = monocular feature) and mbf (rsc_frameview_set_stereo):
        what isInFrustum's mTrackProjXR and the stereo gate of the local-map matcher read."""
        u = np.ascontiguousarray(u_right, np.float32).reshape(-1)
        assert u.size == self.n
        if not self.n:
            u = np.zeros(1, np.float32)
        _check(load_library().rsc_frameview_set_stereo(self.h, u, float(mbf)), "rsc_frameview_set_stereo")

    def compute_stereo(self, right, mbf: float, mb: float, set_stereo: bool = True):
        """Frame::ComputeStereoMatches of this Frame against the right image's features `right` (an object with
        r_kp float32 [m,2], r_octave int32 [m], r_desc uint8 [m,32]); see compute_stereo_matches_many, whose
        result dict for the one frame this returns."""
        return compute_stereo_matches_many(self.ctx, [self], [right], [mbf], [mb], set_stereo)[0]

    def close(self):
        if getattr(self, "h", None):
            load_library().rsc_frameview_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()


def _ptrs(arrays):
    return (C.c_void_p * max(len(arrays), 1))(*[a.ctypes.data for a in arrays])


def _handles(views):
    return (C.c_void_p * max(len(views), 1))(*[v.h.value for v in views])


def search_by_projection_many(ctx: Context, frames, kfs, Tcw, already, frame_mp, th: float, orb_dist: int,
                              check_orientation: bool = True):
    """ORBmatcher::SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist) (ORBmatcher.cpp:1317-1444)
    for each (FrameView, KFView, Tcw [4,4], already uint8 [kf n], frame_mp int32 [frame n]) in one launch.
    Returns (list of out int32 [frame n] = KeyFrame slot of each new match or -1, nmatches int32[count],
    rounds int32[count])."""
    c = len(frames)
    T = np.ascontiguousarray(np.asarray(Tcw, np.float32).reshape(c, 16)) if c else np.zeros((1, 16), np.float32)
    al = [np.ascontiguousarray(a, np.uint8) if k.n else np.zeros(1, np.uint8) for a, k in zip(already, kfs)]
    mp = [np.ascontiguousarray(a, np.int32) if f.n else np.zeros(1, np.int32) for a, f in zip(frame_mp, frames)]
    out = [np.full(max(f.n, 1), -7, np.int32) for f in frames]
    nm = np.zeros(max(c, 1), np.int32)
    rounds = np.zeros(max(c, 1), np.int32)
    _check(load_library().rsc_search_by_projection_many(ctx.h, _handles(frames), _handles(kfs), c, T, _ptrs(al),
                                                        _ptrs(mp), float(th), int(orb_dist), int(check_orientation),
                                                        _ptrs(out), nm, rounds), "rsc_search_by_projection_many")
    return [o[:f.n] for o, f in zip(out, frames)], nm[:c], rounds[:c]


class MapPointsStruct(C.Structure):
    """rsc_mappoints (include/rsc.h)."""
    _fields_ = [("n", C.c_int32), ("state", C.c_void_p), ("pos", C.c_void_p), ("normal", C.c_void_p),
                ("dmax", C.c_void_p), ("dmin", C.c_void_p), ("desc", C.c_void_p)]


class LoopVerifyResult(C.Structure):
    """rsc_loop_verify_result (include/rsc.h)."""
    _fields_ = [("accepted", C.c_int32), ("n_projected", C.c_int32), ("n_total", C.c_int32),
                ("Scw_sim3", C.c_double * 8), ("Scw", C.c_float * 16)]


class MPView:
    """A flat list of distinct MapPoints (mvpLoopMapPoints) resident in HBM (rsc_mpview_create): an object
    with n, state uint8 [n], pos / normal float32 [n,3], dmax / dmin float32 [n], desc uint8 [n,32]."""

    def __init__(self, ctx: Context, pts):
        self.ctx, self.n = ctx, int(pts.n)
        pad = lambda a, dt, k: (np.ascontiguousarray(a, dt).reshape(-1) if self.n else np.zeros(k, dt))
        keep = [pad(pts.state, np.uint8, 1), pad(pts.pos, np.float32, 3), pad(pts.normal, np.float32, 3),
                pad(pts.dmax, np.float32, 1), pad(pts.dmin, np.float32, 1), pad(pts.desc, np.uint8, 32)]
        m = MapPointsStruct()
        m.n = self.n
        m.state, m.pos, m.normal, m.dmax, m.dmin, m.desc = (a.ctypes.data for a in keep)
        h = C.c_void_p()
        _check(load_library().rsc_mpview_create(ctx.h, C.byref(m), C.byref(h)), "rsc_mpview_create")
        self.h = h

    def download(self):
        """The view as it is in HBM now (rsc_mpview_download, a diagnostic): a namespace with n, state, pos, normal,
        dmax, dmin, desc."""
        import types
        n = max(self.n, 1)
        o = types.SimpleNamespace(n=self.n, state=np.zeros(n, np.uint8), pos=np.zeros((n, 3), np.float32),
                                  normal=np.zeros((n, 3), np.float32), dmax=np.zeros(n, np.float32),
                                  dmin=np.zeros(n, np.float32), desc=np.zeros((n, 32), np.uint8))
        _check(load_library().rsc_mpview_download(self.h, o.state, o.pos, o.normal, o.dmax, o.dmin, o.desc),
               "rsc_mpview_download")
        for k in ("state", "pos", "normal", "dmax", "dmin", "desc"):
            setattr(o, k, getattr(o, k)[:self.n])
        return o

    def close(self):
        if getattr(self, "h", None):
            load_library().rsc_mpview_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()


def search_by_projection_kf_many(ctx: Context, kfs, points, Scw, already, occupied, th: int = 10):
    """ORBmatcher::SearchByProjection(pKF, Scw, vpPoints, vpMatched, th) (ORBmatcher.cpp:241-352) for each
    (KFView, MPView, Scw [4,4], already uint8 [points n], occupied uint8 [kf n]) in one launch.  Returns
    (list of out int32 [kf n] = index into the points of the MapPoint written to vpMatched[idx] or -1,
    nmatches int32[count], rounds int32[count])."""
    c = len(kfs)
    S = np.ascontiguousarray(np.asarray(Scw, np.float32).reshape(c, 16)) if c else np.zeros((1, 16), np.float32)
    al = [np.ascontiguousarray(a, np.uint8) if p.n else np.zeros(1, np.uint8) for a, p in zip(already, points)]
    oc = [np.ascontiguousarray(a, np.uint8) if k.n else np.zeros(1, np.uint8) for a, k in zip(occupied, kfs)]
    out = [np.full(max(k.n, 1), -7, np.int32) for k in kfs]
    nm = np.zeros(max(c, 1), np.int32)
    rounds = np.zeros(max(c, 1), np.int32)
    _check(load_library().rsc_search_by_projection_kf_many(ctx.h, _handles(kfs), _handles(points), c, S, _ptrs(al),
                                                           _ptrs(oc), int(th), _ptrs(out), nm, rounds),
           "rsc_search_by_projection_kf_many")
    return [o[:k.n] for o, k in zip(out, kfs)], nm[:c], rounds[:c]


# rsc_track_record (include/rsc.h): what Frame::isInFrustum leaves in a MapPoint
TRACK_RECORD = np.dtype([("in_view", np.int32), ("proj_x", np.float32), ("proj_y", np.float32),
                         ("proj_xr", np.float32), ("level", np.int32), ("view_cos", np.float32)])


def _local_points(ctx, frames, points, Tcw, skip, has_obs, frame_occ, cos_limit, th, nn_ratio, track):
    c = len(frames)
    u8 = lambda arrays, views: [np.ascontiguousarray(a, np.uint8) if v.n else np.zeros(1, np.uint8)
                                for a, v in zip(arrays, views)]
    sk, ho, oc = u8(skip, points), u8(has_obs, points), u8(frame_occ, frames)
    out = [np.full(max(f.n, 1), -7, np.int32) for f in frames]
    if track is None:
        tr = [np.zeros(max(p.n, 1), TRACK_RECORD) for p in points]
    else:
        tr = [np.ascontiguousarray(t, TRACK_RECORD) if p.n else np.zeros(1, TRACK_RECORD)
              for t, p in zip(track, points)]
    nm, ntm, rounds = (np.zeros(max(c, 1), np.int32) for _ in range(3))
    L = load_library()
    if track is None:
        T = np.ascontiguousarray(np.asarray(Tcw, np.float32).reshape(c, 16)) if c else np.zeros((1, 16), np.float32)
        _check(L.rsc_search_local_points_many(ctx.h, _handles(frames), _handles(points), c, T, _ptrs(sk), _ptrs(ho),
                                              _ptrs(oc), float(cos_limit), float(th), float(nn_ratio), _ptrs(out),
                                              _ptrs(tr), nm, ntm, rounds), "rsc_search_local_points_many")
    else:
        _check(L.rsc_search_by_projection_points_many(ctx.h, _handles(frames), _handles(points), c, _ptrs(sk),
                                                      _ptrs(ho), _ptrs(oc), float(th), float(nn_ratio), _ptrs(out),
                                                      _ptrs(tr), nm, ntm, rounds),
               "rsc_search_by_projection_points_many")
    return dict(out=[o[:f.n] for o, f in zip(out, frames)], track=[t[:p.n] for t, p in zip(tr, points)],
                nmatches=nm[:c], n_to_match=ntm[:c], rounds=rounds[:c])


def search_local_points_many(ctx: Context, frames, points, Tcw, skip, has_obs, frame_occ, cos_limit: float = 0.5,
                             th: float = 1.0, nn_ratio: float = 0.8):
    """Tracking::SearchLocalPoints (Tracking.cpp:1003-1028): Frame::isInFrustum over the list, then
    ORBmatcher::SearchByProjection(F, vpMapPoints, th), for each (FrameView with set_stereo, MPView, Tcw [4,4],
    skip uint8 [points n], has_obs uint8 [points n], frame_occ uint8 [frame n]: 0 NULL / 1 set without
    observations / 2 set with observations) in one launch.  Returns a dict of per-problem lists / arrays: out
    (int32 [frame n]: index into the points of the MapPoint left in mvpMapPoints[f], or -1), track
    (TRACK_RECORD [points n]), nmatches, n_to_match, rounds."""
    return _local_points(ctx, frames, points, Tcw, skip, has_obs, frame_occ, cos_limit, th, nn_ratio, None)


def search_by_projection_points_many(ctx: Context, frames, points, track, skip, has_obs, frame_occ, th: float = 1.0,
                                     nn_ratio: float = 0.8):
    """The bare ORBmatcher::SearchByProjection(F, vpMapPoints, th) (ORBmatcher.cpp:16-100) on the host's track
    members (TRACK_RECORD [points n] per problem, not modified); otherwise as search_local_points_many."""
    return _local_points(ctx, frames, points, None, skip, has_obs, frame_occ, 0.0, th, nn_ratio, track)


class LastFrameSlots(C.Structure):
    """rsc_last_frame_slots (include/rsc.h)."""
    _fields_ = [("n", C.c_int32), ("octave", C.c_void_p), ("angle", C.c_void_p), ("mp_state", C.c_void_p),
                ("mp_pos", C.c_void_p), ("mp_desc", C.c_void_p), ("mp_has_obs", C.c_void_p)]


class TrackMotionResult(C.Structure):
    """rsc_track_motion_result (include/rsc.h)."""
    _fields_ = [("ok", C.c_int32), ("searches", C.c_int32), ("nmatches_search", C.c_int32 * 2), ("mode", C.c_int32),
                ("nmatches", C.c_int32), ("nmatches_map", C.c_int32), ("vo", C.c_int32), ("n_good", C.c_int32),
                ("Tcw", C.c_float * 16)]


class LastFrameView:
    """The last Frame as the motion-model matcher reads it, resident in HBM (rsc_lastframe_create): an object
    with n, octave int32 [n] (mvKeys), angle float32 [n] (mvKeysUn), mp_state uint8 [n] (0 NULL, 1 set, 2 set
    and mvbOutlier), mp_pos float32 [n,3], mp_desc uint8 [n,32] (MapPoint::GetDescriptor), mp_has_obs uint8 [n]."""

    def __init__(self, ctx: Context, last):
        self.ctx, self.n = ctx, int(last.n)
        pad = lambda a, dt, k: (np.ascontiguousarray(a, dt).reshape(-1) if self.n else np.zeros(k, dt))
        keep = [pad(last.octave, np.int32, 1), pad(last.angle, np.float32, 1), pad(last.mp_state, np.uint8, 1),
                pad(last.mp_pos, np.float32, 3), pad(last.mp_desc, np.uint8, 32), pad(last.mp_has_obs, np.uint8, 1)]
        m = LastFrameSlots()
        m.n = self.n
        m.octave, m.angle, m.mp_state, m.mp_pos, m.mp_desc, m.mp_has_obs = (a.ctypes.data for a in keep)
        h = C.c_void_p()
        _check(load_library().rsc_lastframe_create(ctx.h, C.byref(m), C.byref(h)), "rsc_lastframe_create")
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            load_library().rsc_lastframe_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()


def _poses(T, c):
    return np.ascontiguousarray(np.asarray(T, np.float32).reshape(c, 16)) if c else np.zeros((1, 16), np.float32)


def search_by_projection_last_many(ctx: Context, frames, lasts, Tcw_cur, Tcw_last, mb, frame_occ=None,
                                   th: float = 7.0, check_orientation: bool = True):
    """ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th) (ORBmatcher.cpp:1173-1315) for each (FrameView
    with set_stereo, LastFrameView, Tcw_cur [4,4], Tcw_last [4,4], mb, frame_occ uint8 [frame n] or None = all
    NULL) in one launch.  Returns a dict of per-problem lists / arrays: out (int32 [frame n]: >= 0 the LastFrame
    slot left in mvpMapPoints[f], -1 untouched, -2 set to nullptr by the rotation check), nmatches, mode (0
    window, 1 forward, 2 backward), rounds."""
    c = len(frames)
    if frame_occ is None:
        frame_occ = [None] * c
    oc = [np.zeros(max(f.n, 1), np.uint8) if a is None or not f.n else np.ascontiguousarray(a, np.uint8)
          for a, f in zip(frame_occ, frames)]
    out = [np.full(max(f.n, 1), -7, np.int32) for f in frames]
    nm, mode, rounds = (np.zeros(max(c, 1), np.int32) for _ in range(3))
    b = np.ascontiguousarray(mb, np.float32).reshape(-1) if c else np.zeros(1, np.float32)
    assert b.size == max(c, 1)
    _check(load_library().rsc_search_by_projection_last_many(
        ctx.h, _handles(frames), _handles(lasts), c, _poses(Tcw_cur, c), _poses(Tcw_last, c), b, _ptrs(oc),
        float(th), int(check_orientation), _ptrs(out), nm, mode, rounds), "rsc_search_by_projection_last_many")
    return dict(out=[o[:f.n] for o, f in zip(out, frames)], nmatches=nm[:c], mode=mode[:c], rounds=rounds[:c])


def track_motion_model_many(ctx: Context, frames, lasts, Tcw_cur, Tcw_last, mb, th: float = 7.0,
                            only_tracking=None):
    """Tracking::TrackWithMotionModel (Tracking.cpp:724-774, rsc_track_motion_model_many) for each (FrameView
    with set_stereo, LastFrameView after UpdateLastFrame, Tcw_cur = mVelocity * mLastFrame.mTcw, Tcw_last, mb,
    only_tracking = mbOnlyTracking per frame, default all false).  Returns (TrackMotionResult records, list of out
    int32 [frame n] after the discard, list of discarded int32 [frame n])."""
    c = len(frames)
    out = [np.full(max(f.n, 1), -7, np.int32) for f in frames]
    disc = [np.full(max(f.n, 1), -7, np.int32) for f in frames]
    b = np.ascontiguousarray(mb, np.float32).reshape(-1) if c else np.zeros(1, np.float32)
    assert b.size == max(c, 1)
    res = (TrackMotionResult * max(c, 1))()
    ot = np.zeros(max(c, 1), np.int32)
    if only_tracking is not None and c:
        ot[:] = np.asarray(only_tracking, np.int32).reshape(c)
    _check(load_library().rsc_track_motion_model_many(
        ctx.h, _handles(frames), _handles(lasts), c, _poses(Tcw_cur, c), _poses(Tcw_last, c), b, float(th),
        ot, res, _ptrs(out), _ptrs(disc)), "rsc_track_motion_model_many")
    return (np.ctypeslib.as_array(res).copy()[:c], [o[:f.n] for o, f in zip(out, frames)],
            [d[:f.n] for d, f in zip(disc, frames)])


def _opt_flags(flags, views):
    """Per-call uint8 [n] flag arrays (entries may be None) as a pointer table, or None for the whole argument."""
    if flags is None:
        return None, []
    keep = [None if a is None else (np.ascontiguousarray(a, np.uint8) if v.n else np.zeros(1, np.uint8))
            for a, v in zip(flags, views)]
    return (C.c_void_p * max(len(keep), 1))(*[None if a is None else a.ctypes.data for a in keep]), keep


def search_for_triangulation_many(ctx: Context, bow1, kf1, bow2, kf2, F12, has_mp1=None, has_mp2=None,
                                  only_stereo: bool = False, check_orientation: bool = False):
    """ORBmatcher::SearchForTriangulation (ORBmatcher.cpp:489-669) for each (BowView, KFView of KeyFrame 1, BowView,
    KFView of KeyFrame 2, F12 [3,3]) in one launch; the KFViews carry set_triangulation.  has_mp1 / has_mp2: lists
    of uint8 [n] (GetMapPoint(idx) != nullptr) or None = the views' mp_state != 0; only_stereo: one bool or one per
    problem.  Returns a dict: matches12 (list
    of int32 [n1]: KeyFrame-2 index or -1), nmatches, den_zero (int32 [count]), den_zero_slot (list of uint8 [n1])."""
    c = len(kf1)
    F = np.ascontiguousarray(np.asarray(F12, np.float32).reshape(c, 9)) if c else np.zeros((1, 9), np.float32)
    out = [np.full(max(k.n, 1), -7, np.int32) for k in kf1]
    dzs = [np.full(max(k.n, 1), 7, np.uint8) for k in kf1]
    nm, dz = (np.full(max(c, 1), -7, np.int32) for _ in range(2))
    os_ = np.zeros(max(c, 1), np.int32)
    os_[:c] = np.asarray(only_stereo, np.int32)  # one value, or one per problem
    h1, keep1 = _opt_flags(has_mp1, kf1)
    h2, keep2 = _opt_flags(has_mp2, kf2)
    _check(load_library().rsc_search_for_triangulation_many(
        ctx.h, _handles(bow1), _handles(kf1), _handles(bow2), _handles(kf2), c, F, h1, h2, os_,
        int(check_orientation), _ptrs(out), nm, dz, _ptrs(dzs)), "rsc_search_for_triangulation_many")
    return dict(matches12=[o[:k.n] for o, k in zip(out, kf1)], nmatches=nm[:c], den_zero=dz[:c],
                den_zero_slot=[d[:k.n] for d, k in zip(dzs, kf1)])


def triangulate_pairs_many(ctx: Context, kf1, kf2, pairs):
    """The pair geometry of LocalMapping::CreateNewMapPoints (LocalMapping.cpp:262-407) for each (KFView of the
    current KeyFrame, KFView of the neighbour, pairs int32 [np,2]).  Returns (list of status int32 [np], list of
    x3d float32 [np,3])."""
    c = len(kf1)
    pr = [np.ascontiguousarray(p, np.int32).reshape(-1, 2) for p in pairs]
    npairs = np.array([len(p) for p in pr] or [0], np.int32)
    pr = [p if len(p) else np.zeros((1, 2), np.int32) for p in pr]
    st = [np.full(max(int(n), 1), -7, np.int32) for n in npairs[:c]]
    x = [np.full((max(int(n), 1), 3), np.nan, np.float32) for n in npairs[:c]]
    _check(load_library().rsc_triangulate_pairs_many(ctx.h, _handles(kf1), _handles(kf2), c, npairs, _ptrs(pr),
                                                      _ptrs(st), _ptrs(x)), "rsc_triangulate_pairs_many")
    return [s[:n] for s, n in zip(st, npairs)], [a[:n] for a, n in zip(x, npairs)]


def create_new_map_points_many(ctx: Context, bow_cur, kf_cur, bow_neigh, kf_neigh):
    """LocalMapping::CreateNewMapPoints' neighbour loop (LocalMapping.cpp:224-428, rsc_create_new_map_points_many)
    for each current KeyFrame (BowView, KFView) with its ordered neighbour lists bow_neigh[c] / kf_neigh[c].
    Returns a dict of per-KeyFrame lists: new_neighbour int32 [n] (-1 = none), new_idx2 int32 [n], new_pos float32
    [n,3], and nnew int32 [count]."""
    c = len(kf_cur)
    begin = np.zeros(c + 1, np.int32)
    begin[1:] = np.cumsum([len(k) for k in kf_neigh])
    fb = [b for bs in bow_neigh for b in bs]
    fk = [k for ks in kf_neigh for k in ks]
    nn = [np.full(max(k.n, 1), -7, np.int32) for k in kf_cur]
    i2 = [np.full(max(k.n, 1), -7, np.int32) for k in kf_cur]
    pos = [np.full((max(k.n, 1), 3), np.nan, np.float32) for k in kf_cur]
    nnew = np.full(max(c, 1), -7, np.int32)
    _check(load_library().rsc_create_new_map_points_many(ctx.h, _handles(bow_cur), _handles(kf_cur), c, begin,
                                                          _handles(fb), _handles(fk), _ptrs(nn), _ptrs(i2), _ptrs(pos),
                                                          nnew), "rsc_create_new_map_points_many")
    return dict(new_neighbour=[a[:k.n] for a, k in zip(nn, kf_cur)], new_idx2=[a[:k.n] for a, k in zip(i2, kf_cur)],
                new_pos=[a[:k.n] for a, k in zip(pos, kf_cur)], nnew=nnew[:c])


def fuse_sim3_many(ctx: Context, kfs, points, Scw, in_kf, th: float):
    """ORBmatcher::Fuse(pKF, Scw, vpPoints, th, vpReplacePoint) (ORBmatcher.cpp:823-946) for each (KFView,
    Scw [4,4] with linear() = s R, in_kf uint8 [points n]) against one MPView in one launch.  Returns (list of
    best_idx int32 [points n], nfused int32[count])."""
    c = len(kfs)
    S = np.ascontiguousarray(np.asarray(Scw, np.float32).reshape(c, 16)) if c else np.zeros((1, 16), np.float32)
    ik = [np.ascontiguousarray(a, np.uint8) if points.n else np.zeros(1, np.uint8) for a in in_kf]
    best = [np.full(max(points.n, 1), -7, np.int32) for _ in kfs]
    nf = np.zeros(max(c, 1), np.int32)
    _check(load_library().rsc_fuse_sim3_many(ctx.h, _handles(kfs), c, points.h, S, _ptrs(ik), float(th),
                                             _ptrs(best), nf), "rsc_fuse_sim3_many")
    return [b[:points.n] for b in best], nf[:c]


def fuse_kf_many(ctx: Context, kfs, points, skip, th: float):
    """ORBmatcher::Fuse(pKF, vpMapPoints, th) (ORBmatcher.cpp:671-821), the matcher of
    LocalMapping::SearchInNeighbors, for each (KFView with set_triangulation, MPView, skip uint8 [points n] =
    isBad() || IsInKeyFrame(pKF)) in one launch; `points` may name one MPView several times.  Returns (list of
    best_idx int32 [points n], nfused int32[count]); the bookkeeping of :797-817 stays with the caller."""
    c = len(kfs)
    sk = [np.ascontiguousarray(a, np.uint8) if p.n else np.zeros(1, np.uint8) for a, p in zip(skip, points)]
    best = [np.full(max(p.n, 1), -7, np.int32) for p in points]
    nf = np.zeros(max(c, 1), np.int32)
    _check(load_library().rsc_fuse_kf_many(ctx.h, _handles(kfs), _handles(points), c, _ptrs(sk), float(th),
                                           _ptrs(best), nf), "rsc_fuse_kf_many")
    return [b[:p.n] for b, p in zip(best, points)], nf[:c]


class MapPointUpdates(C.Structure):
    """rsc_mappoint_updates (include/rsc.h)."""
    _fields_ = [("n_points", C.c_int32), ("skip", C.c_void_p), ("pos", C.c_void_p), ("obs_begin", C.c_void_p),
                ("obs_kf", C.c_void_p), ("obs_idx", C.c_void_p), ("kf_bad", C.c_void_p), ("ref_kf", C.c_void_p),
                ("ref_idx", C.c_void_p)]


class MapPointUpdateOut(C.Structure):
    """rsc_mappoint_update_out (include/rsc.h)."""
    _fields_ = [("desc", C.c_void_p), ("best_obs", C.c_void_p), ("normal", C.c_void_p), ("dmax", C.c_void_p),
                ("dmin", C.c_void_p), ("updated", C.c_void_p)]


MPUPDATE_MAX_OBS = 1024  # RSC_MPUPDATE_MAX_OBS
# what update_map_points_many puts into the entries the call does not write
MPUPDATE_FILL = dict(desc=0xA5, best_obs=-7, normal=np.float32(-77.0), dmax=np.float32(-77.0), dmin=np.float32(-77.0))


def update_map_points_many(ctx: Context, kfs, updates, what: int = 3, dst=None, dst_index=None, out=None):
    """MapPoint::ComputeDistinctiveDescriptors (what & 1) and MapPoint::UpdateNormalAndDepth (what & 2)
    (MapPoint.cpp:224-289, :312-353; rsc_update_map_points_many) for a batch of points over the KFViews `kfs`
    (with set_triangulation for what & 2).  `updates`: an object with n_points, skip uint8 [n], pos float32 [n,3],
    obs_begin int32 [n+1], obs_kf / obs_idx int32 [n_obs], kf_bad uint8 [len(kfs)] or None, ref_kf / ref_idx int32
    [n].  dst / dst_index: an MPView and int32 [n] slots (-1: none) that receive the written fields on the device.
    Returns a dict: desc uint8 [n,32], best_obs int32 [n], normal float32 [n,3], dmax, dmin float32 [n], updated
    uint8 [n]; entries the call did not write hold MPUPDATE_FILL.  out: such a dict to write into instead (entries
    not written keep what it holds, and a refused call leaves it as it is)."""
    n = int(updates.n_points)
    m = max(n, 1)
    arr = lambda a, dt, k: (np.ascontiguousarray(a, dt).reshape(-1) if a is not None and np.size(a) else np.zeros(k, dt))
    keep = dict(skip=arr(updates.skip, np.uint8, m), pos=arr(updates.pos, np.float32, 3 * m),
                obs_begin=arr(updates.obs_begin if n else None, np.int32, m + 1), obs_kf=arr(updates.obs_kf, np.int32, 1),
                obs_idx=arr(updates.obs_idx, np.int32, 1), ref_kf=arr(updates.ref_kf, np.int32, m),
                ref_idx=arr(updates.ref_idx, np.int32, m))
    assert keep["obs_begin"].size == m + 1 and keep["pos"].size == 3 * m and keep["skip"].size == m
    u = MapPointUpdates()
    u.n_points = n
    for k, a in keep.items():
        setattr(u, k, a.ctypes.data)
    bad = getattr(updates, "kf_bad", None)
    if bad is not None:
        bad = arr(bad, np.uint8, 1)
        assert bad.size >= len(kfs)
        u.kf_bad = bad.ctypes.data
    F = MPUPDATE_FILL
    res = dict(desc=np.full((m, 32), F["desc"], np.uint8), best_obs=np.full(m, F["best_obs"], np.int32),
               normal=np.full((m, 3), F["normal"], np.float32), dmax=np.full(m, F["dmax"], np.float32),
               dmin=np.full(m, F["dmin"], np.float32), updated=np.full(m, 0xFF, np.uint8))
    if out is not None:
        assert all(out[k].dtype == a.dtype and out[k].size >= a[:n].size and out[k].flags.c_contiguous
                   for k, a in res.items())
        res = out
    o = MapPointUpdateOut()
    for k, a in res.items():
        setattr(o, k, a.ctypes.data)
    di = None
    if dst is not None:
        di = arr(dst_index, np.int32, m)
        assert di.size == m
    _check(load_library().rsc_update_map_points_many(ctx.h, _handles(kfs), len(kfs), C.byref(u), int(what),
                                                      C.byref(o), dst.h if dst is not None else None,
                                                      di.ctypes.data if di is not None else None),
           "rsc_update_map_points_many")
    return res if out is not None else {k: a[:n] for k, a in res.items()}


class LocalBAProblem(C.Structure):
    """rsc_localba_problem (include/rsc.h)."""
    _fields_ = [("n_kfs", C.c_int32), ("kf_id", C.c_void_p), ("fixed", C.c_void_p), ("Tcw", C.c_void_p),
                ("cam", C.c_void_p), ("n_points", C.c_int32), ("mp_id", C.c_void_p), ("pos", C.c_void_p),
                ("bad", C.c_void_p), ("obs_begin", C.c_void_p), ("obs_kf", C.c_void_p), ("uv", C.c_void_p),
                ("u_right", C.c_void_p), ("inv_sigma2", C.c_void_p)]


class LocalBAOut(C.Structure):
    """rsc_localba_out (include/rsc.h)."""
    _fields_ = [("Tcw", C.c_void_p), ("pos", C.c_void_p), ("edge_flags", C.c_void_p), ("erase", C.c_void_p)]


class LocalBAPhase(C.Structure):
    """rsc_localba_phase (include/rsc.h)."""
    _fields_ = [("n_vertices", C.c_int32), ("n_points", C.c_int32), ("n_edges", C.c_int32),
                ("lm_iterations", C.c_int32), ("lm_trials", C.c_int32), ("chi2_first", C.c_double),
                ("chi2_last", C.c_double)]


class LocalBAResult(C.Structure):
    """rsc_localba_result (include/rsc.h)."""
    _fields_ = [("n_erase", C.c_int32), ("n_level1", C.c_int32), ("status", C.c_int32), ("phase", LocalBAPhase * 2),
                ("branches", C.c_int32 * 12)]


LOCALBA_MAX_FREE_KFS, LOCALBA_MAX_KFS, LOCALBA_MAX_POINTS, LOCALBA_MAX_EDGES = 64, 4160, 16384, 131072
LOCALBA_BRANCHES = ("iterations", "trials", "zero_pivot", "chi_non_finite", "rho_nan", "rejected", "qmax", "rho_zero",
                    "nbad", "no_active_edge", "vertex_dropped", "stale_kept")
# what local_bundle_adjustment puts into its outputs before the call (a refused call leaves them)
LOCALBA_FILL = dict(Tcw=np.float32(-77.0), pos=np.float32(-77.0), edge_flags=0xA5, erase=-7)


def localba_pack(problem):
    """The ctypes image of a LocalBundleAdjustment problem: a dict (rsc/synth.make_localba_scene's keys kf_id int64
    [K], fixed uint8 [K], Tcw float32 [K,16], cam float32 [K,5], mp_id int64 [N], pos float32 [N,3], bad uint8 [N],
    obs_begin int32 [N+1], obs_kf int32 [E], uv float32 [E,2], u_right float32 [E], inv_sigma2 float32 [E]).
    Returns (LocalBAProblem, the arrays it points at)."""
    dt = dict(kf_id=np.int64, fixed=np.uint8, Tcw=np.float32, cam=np.float32, mp_id=np.int64, pos=np.float32,
              bad=np.uint8, obs_begin=np.int32, obs_kf=np.int32, uv=np.float32, u_right=np.float32, inv_sigma2=np.float32)
    keep = {}
    for k, t in dt.items():
        a = np.ascontiguousarray(problem[k], t).reshape(-1)
        keep[k] = a if a.size else np.zeros(1, t)
    q = LocalBAProblem()
    q.n_kfs = int(np.size(problem["kf_id"]))
    q.n_points = int(np.size(problem["mp_id"]))
    for k, a in keep.items():
        setattr(q, k, a.ctypes.data)
    return q, keep


def localba_outputs(problem):
    """Output arrays of one problem, holding LOCALBA_FILL."""
    K, N = int(np.size(problem["kf_id"])), int(np.size(problem["mp_id"]))
    E = int(np.size(problem["obs_kf"]))
    F = LOCALBA_FILL
    return dict(Tcw=np.full((max(K, 1), 16), F["Tcw"], np.float32), pos=np.full((max(N, 1), 3), F["pos"], np.float32),
                edge_flags=np.full(max(E, 1), F["edge_flags"], np.uint8), erase=np.full(max(E, 1), F["erase"], np.int32))


def localba_result_dict(problem, arrays, r):
    """What a LocalBundleAdjustment call returned, as a dict (arrays cut to the problem's sizes)."""
    K, N = int(np.size(problem["kf_id"])), int(np.size(problem["mp_id"]))
    E = int(np.size(problem["obs_kf"]))
    ph = [dict(n_vertices=p.n_vertices, n_points=p.n_points, n_edges=p.n_edges, lm_iterations=p.lm_iterations,
               lm_trials=p.lm_trials, chi2_first=np.float64(p.chi2_first), chi2_last=np.float64(p.chi2_last))
          for p in r.phase]
    return dict(Tcw=arrays["Tcw"][:K], pos=arrays["pos"][:N], edge_flags=arrays["edge_flags"][:E],
                erase=arrays["erase"][:r.n_erase].copy(), n_erase=r.n_erase, n_level1=r.n_level1, status=r.status,
                phase=ph, branches=dict(zip(LOCALBA_BRANCHES, list(r.branches))))


def local_bundle_adjustment_many(ctx: Context, problems):
    """Optimizer::LocalBundleAdjustment (Optimizer.cpp:426-787; rsc_local_bundle_adjustment_many) on each problem
    dict (localba_pack's keys).  Returns one dict per problem: Tcw float32 [K,16], pos float32 [N,3], edge_flags
    uint8 [E] (bit 0 level 1 after the first optimize(), bit 1 in vToErase), erase int32 [n_erase], n_erase,
    n_level1, status, phase (two dicts), branches."""
    c = len(problems)
    packed = [localba_pack(p) for p in problems]
    arrays = [localba_outputs(p) for p in problems]
    P = (LocalBAProblem * max(c, 1))(*[q for q, _ in packed])
    O = (LocalBAOut * max(c, 1))()
    for i, a in enumerate(arrays):
        for k, v in a.items():
            setattr(O[i], k, v.ctypes.data)
    R = (LocalBAResult * max(c, 1))()
    _check(load_library().rsc_local_bundle_adjustment_many(ctx.h, P, c, O, R), "rsc_local_bundle_adjustment_many")
    return [localba_result_dict(p, a, r) for p, a, r in zip(problems, arrays, R)]


LOCALBA_STAGES = ("build", "vertex_sums", "iteration_head", "point_inverses", "schur", "reduced_solve", "trial_errors",
                  "update", "trial_tail", "restore", "classify")


def localba_stage_ms(ctx: Context):
    """Device milliseconds per stage of the last local_bundle_adjustment* call that ran with timing on
    (rsc_diag_localba_stages), as a dict over LOCALBA_STAGES."""
    out = (C.c_double * 11)()
    _check(load_library().rsc_diag_localba_stages(ctx.h, out, 11), "rsc_diag_localba_stages")
    return dict(zip(LOCALBA_STAGES, [float(v) for v in out]))


def local_bundle_adjustment(ctx: Context, problem):
    """local_bundle_adjustment_many on one problem."""
    return local_bundle_adjustment_many(ctx, [problem])[0]


class RightFeatures(C.Structure):
    """rsc_right_features (include/rsc.h)."""
    _fields_ = [("n", C.c_int32), ("kp", C.c_void_p), ("octave", C.c_void_p), ("desc", C.c_void_p)]


class StereoResult(C.Structure):
    """rsc_stereo_result (include/rsc.h)."""
    _fields_ = [("n_candidates", C.c_int32), ("n_removed", C.c_int32), ("median", C.c_int32), ("th_dist", C.c_float)]


STEREO_MAX_RIGHT = 8192  # RSC_STEREO_MAX_RIGHT
# what compute_stereo_matches_many puts into its outputs before the call (a refused call leaves them)
STEREO_FILL = dict(u_right=np.float32(-77.0), depth=np.float32(-77.0), best_right=-7, best_dist=-7)


def compute_stereo_matches_many(ctx: Context, frames, rights, mbf, mb, set_stereo: bool = True,
                                diagnostics: bool = True, out=None):
    """Frame::ComputeStereoMatches (Frame.cpp:538-673; rsc_compute_stereo_matches_many) for each (FrameView,
    right features) pair in one launch per phase.  rights[c]: an object with r_kp float32 [m,2] (mvKeysRight pt, as
    extracted), r_octave int32 [m], r_desc uint8 [m,32]; mbf / mb: one float per frame.  set_stereo leaves every
    view as FrameView.set_stereo(u_right, mbf) would, without an upload.  Returns one dict per frame: u_right,
    depth float32 [n] (mvuRight, mvDepth), best_right, best_dist int32 [n] (before the cut, -1: not accepted; None
    without `diagnostics`), n_candidates, n_removed, median, th_dist.  out: a list of such dicts of arrays to write
    into instead (a refused call leaves them as they are)."""
    c = len(frames)
    assert len(rights) == c
    keep, R = [], (RightFeatures * max(c, 1))()
    for k, r in enumerate(rights):
        a = [np.ascontiguousarray(r.r_kp, np.float32).reshape(-1), np.ascontiguousarray(r.r_octave, np.int32).reshape(-1),
             np.ascontiguousarray(r.r_desc, np.uint8).reshape(-1)]
        assert a[0].size == 2 * a[1].size and a[2].size == 32 * a[1].size
        R[k].n = a[1].size
        a = [x if x.size else np.zeros(32, x.dtype) for x in a]
        R[k].kp, R[k].octave, R[k].desc = (x.ctypes.data for x in a)
        keep.append(a)
    F = STEREO_FILL
    if out is None:
        out = [dict(u_right=np.full(max(f.n, 1), F["u_right"], np.float32), depth=np.full(max(f.n, 1), F["depth"], np.float32),
                    best_right=np.full(max(f.n, 1), F["best_right"], np.int32) if diagnostics else None,
                    best_dist=np.full(max(f.n, 1), F["best_dist"], np.int32) if diagnostics else None) for f in frames]
    res = (StereoResult * max(c, 1))()
    fm = np.ascontiguousarray(mbf, np.float32).reshape(-1) if c else np.zeros(1, np.float32)
    fb = np.ascontiguousarray(mb, np.float32).reshape(-1) if c else np.zeros(1, np.float32)
    assert fm.size == max(c, 1) and fb.size == max(c, 1)
    diag = lambda k: (C.c_void_p * max(c, 1))(*[o[k].ctypes.data if o[k] is not None else None for o in out]) \
        if diagnostics else None
    _check(load_library().rsc_compute_stereo_matches_many(
        ctx.h, _handles(frames), R, c, fm, fb, int(bool(set_stereo)), _ptrs([o["u_right"] for o in out]),
        _ptrs([o["depth"] for o in out]), diag("best_right"), diag("best_dist"), res), "rsc_compute_stereo_matches_many")
    ret = []
    for f, o, r in zip(frames, out, res):
        d = {k: (a[:f.n] if a is not None else None) for k, a in o.items() if k in F}
        d.update(n_candidates=int(r.n_candidates), n_removed=int(r.n_removed), median=int(r.median),
                 th_dist=np.float32(r.th_dist))
        ret.append(d)
    return ret


def loop_verify_many(ctx: Context, kf_cur, kf_matched, loop_points, S, matches, already):
    """The closing stage of LoopClosing::ComputeSim3 (LoopClosing.cpp:318-320, :360-370;
    rsc_loop_verify_many) on the result of the gated loop events: S [count][8] = LoopGateResult.S,
    matches[c] int32 [kf_cur n] = matches_out of the gate, already[c] uint8 [points n].  Returns
    (LoopVerifyResult records, list of projected int32 [kf_cur n])."""
    c = len(kf_cur)
    Sd = np.ascontiguousarray(np.asarray(S, np.float64).reshape(c, 8)) if c else np.zeros((1, 8), np.float64)
    mt = [np.ascontiguousarray(a, np.int32) if k.n else np.full(1, -1, np.int32) for a, k in zip(matches, kf_cur)]
    al = [np.ascontiguousarray(a, np.uint8) if p.n else np.zeros(1, np.uint8) for a, p in zip(already, loop_points)]
    proj = [np.full(max(k.n, 1), -7, np.int32) for k in kf_cur]
    res = (LoopVerifyResult * max(c, 1))()
    _check(load_library().rsc_loop_verify_many(ctx.h, _handles(kf_cur), _handles(kf_matched), _handles(loop_points),
                                               c, Sd, _ptrs(mt), _ptrs(al), res, _ptrs(proj)),
           "rsc_loop_verify_many")
    return [res[k] for k in range(c)], [p[:k.n] for p, k in zip(proj, kf_cur)]


def reloc_refine_many(ctx: Context, frames, kfs, fr, frame_mp, found, n_good_in, Tcw_in):
    """Tracking::Relocalization's refinement chain (Tracking.cpp:1294-1323, rsc_reloc_refine_many) for each
    candidate: fr[c] = (u_right float32 [frame n] or None, bf); frame_mp[c] int32 [frame n] (entry state,
    not modified); found[c] uint8 [kf n]; n_good_in[c]; Tcw_in[c] [4,4].  Returns (RelocRefineResult
    records, list of final frame_mp arrays)."""
    c = len(frames)
    rf = (RelocFrame * max(c, 1))()
    keep = []
    for e, (ur, bf) in enumerate(fr):
        if ur is not None:
            a = np.ascontiguousarray(ur, np.float32)
            keep.append(a)
            rf[e].u_right = a.ctypes.data
        rf[e].bf = float(bf)
    mp = [np.array(a, np.int32) if f.n else np.full(1, -1, np.int32) for a, f in zip(frame_mp, frames)]
    fd = [np.ascontiguousarray(a, np.uint8) if k.n else np.zeros(1, np.uint8) for a, k in zip(found, kfs)]
    ng = np.ascontiguousarray(n_good_in, np.int32).reshape(-1) if c else np.zeros(1, np.int32)
    T = np.ascontiguousarray(np.asarray(Tcw_in, np.float32).reshape(c, 16)) if c else np.zeros((1, 16), np.float32)
    res = (RelocRefineResult * max(c, 1))()
    _check(load_library().rsc_reloc_refine_many(ctx.h, _handles(frames), _handles(kfs), c, rf, _ptrs(mp), _ptrs(fd),
                                                ng, T, res), "rsc_reloc_refine_many")
    return np.ctypeslib.as_array(res).copy()[:c], [m[:f.n] for m, f in zip(mp, frames)]


class Sim3Search:
    """Prepared ORBmatcher::SearchBySim3 batch (ORBmatcher.cpp:948-1170): count (kf1, kf2, R12, t12,
    matched12) problems in one launch over resident KeyFrame views, threshold th (7.5 in
    LoopClosing.cpp:309).  The same KeyFrame object is uploaded once."""

    def __init__(self, ctx: Context, problems, th: float = 7.5):
        self.ctx, self.th = ctx, float(th)
        c = len(problems)
        self.count = c
        self.views = {}
        for p in problems:
            for kf in (p[0], p[1]):
                if id(kf) not in self.views:
                    self.views[id(kf)] = KFView(ctx, kf)
        self.h1 = (C.c_void_p * max(c, 1))(*[self.views[id(p[0])].h.value for p in problems])
        self.h2 = (C.c_void_p * max(c, 1))(*[self.views[id(p[1])].h.value for p in problems])
        self.R = np.ascontiguousarray(np.stack([np.asarray(p[2], np.float32).reshape(9) for p in problems]))
        self.t = np.ascontiguousarray(np.stack([np.asarray(p[3], np.float32).reshape(3) for p in problems]))
        self.m_in = [np.ascontiguousarray(p[4], np.int32) for p in problems]
        self.out = [np.full(max(p[0].n, 1), -7, np.int32) for p in problems]
        self.pin = (C.c_void_p * max(c, 1))(*[a.ctypes.data for a in self.m_in])
        self.pout = (C.c_void_p * max(c, 1))(*[a.ctypes.data for a in self.out])
        self.nfound = np.zeros(max(c, 1), np.int32)
        self.n1 = [p[0].n for p in problems]
        self.n2 = [p[1].n for p in problems]

    def run(self):
        _check(load_library().rsc_search_by_sim3_many(self.ctx.h, self.h1, self.h2, self.count, self.R, self.t,
                                                      self.th, self.pin, self.pout, self.nfound),
               "rsc_search_by_sim3_many")
        return [o[:n] for o, n in zip(self.out, self.n1)], self.nfound[:self.count]

    def directions(self, k: int):
        """(m1 int32[kf1.n] = vnMatch1, m2 int32[kf2.n] = vnMatch2) of pair k as the context's most recent
        SearchBySim3 call left them, before the agreement step (rsc_diag_sim3match_directions)."""
        n1 = self.n1[k] if 0 <= k < self.count else 0
        n2 = self.n2[k] if 0 <= k < self.count else 0
        m1, m2 = np.full(max(n1, 1), -7, np.int32), np.full(max(n2, 1), -7, np.int32)
        _check(load_library().rsc_diag_sim3match_directions(self.ctx.h, int(k), m1, n1, m2, n2),
               "rsc_diag_sim3match_directions")
        return m1[:n1], m2[:n2]


def search_by_sim3_many(ctx: Context, problems, th: float = 7.5):
    """SearchBySim3 for each (kf1, kf2, R12, t12, matched12): returns (list of out12 int32 arrays =
    new match's KF2 keypoint or -1, nfound int32[count])."""
    return Sim3Search(ctx, problems, th).run()


class KeyFrameDatabase:
    """Device-resident KeyFrameDatabase (src/KeyFrameDatabase.cpp, rsc_kfdb_*): KeyFrames are slots
    in [0, capacity); each BowVector is (word ids ascending uint32, values float64).  The per-
    KeyFrame query state (mnLoopQuery/Words/Score, mnRelocQuery/Words/Score) persists across
    queries as in the reference."""

    def __init__(self, ctx: Context, capacity: int, max_words: int = 4096, vocab_words: int = 10 ** 6):
        self.ctx, self.capacity = ctx, int(capacity)
        h = C.c_void_p()
        _check(load_library().rsc_kfdb_create(ctx.h, int(vocab_words), self.capacity, int(max_words), C.byref(h)),
               "rsc_kfdb_create")
        self.h = h
        self._cand = np.zeros(max(self.capacity, 1), np.int32)
        self._n = np.zeros(1, np.int32)

    @staticmethod
    def _bow(ids, vals):
        return np.ascontiguousarray(ids, np.uint32), np.ascontiguousarray(vals, np.float64)

    def add(self, kf: int, ids, vals):
        i, v = self._bow(ids, vals)
        _check(load_library().rsc_kfdb_add(self.h, int(kf), len(i), i, v), "rsc_kfdb_add")

    def erase(self, kf: int):
        _check(load_library().rsc_kfdb_erase(self.h, int(kf)), "rsc_kfdb_erase")

    def release(self, kf: int):
        """Free slot kf for reuse (erase + fresh query state and covisibility row)."""
        _check(load_library().rsc_kfdb_release(self.h, int(kf)), "rsc_kfdb_release")

    def clear(self):
        _check(load_library().rsc_kfdb_clear(self.h), "rsc_kfdb_clear")

    def set_covisibility(self, kf: int, best):
        b = np.ascontiguousarray(best, np.int32)
        _check(load_library().rsc_kfdb_set_covisibility(self.h, int(kf), len(b), b), "rsc_kfdb_set_covisibility")

    def set_covisibility_many(self, kfs, bests):
        """set_covisibility for many slots in one upload (bests: sequences of <= 10 slots)."""
        k = np.ascontiguousarray(kfs, np.int32)
        n = np.array([len(b) for b in bests], np.int32)
        tab = np.zeros((max(len(k), 1), 10), np.int32)
        for i, b in enumerate(bests):
            tab[i, :len(b)] = b
        _check(load_library().rsc_kfdb_set_covisibility_many(self.h, len(k), k, n, tab), "set_covisibility_many")

    def set_covisibility_table(self, kfs, counts, table):
        """set_covisibility_many with the rows already packed: kfs int32 [c], counts int32 [c],
        table int32 [c, 10] (what a C++ caller passes; no per-row Python work)."""
        _check(load_library().rsc_kfdb_set_covisibility_many(self.h, len(kfs), kfs, counts, table),
               "set_covisibility_many")

    def detect_relocalization(self, frame_id: int, ids, vals) -> np.ndarray:
        """DetectRelocalizationCandidates(F) (:174-283): candidate slots in the reference's order."""
        i, v = self._bow(ids, vals)
        _check(load_library().rsc_kfdb_detect_relocalization(self.h, int(frame_id), len(i), i, v, self._cand,
                                                              self._n), "rsc_kfdb_detect_relocalization")
        return self._cand[:self._n[0]].copy()

    def detect_loop(self, kf_id: int, ids, vals, connected, min_score: float) -> np.ndarray:
        """DetectLoopCandidates(pKF, minScore) (:52-172)."""
        i, v = self._bow(ids, vals)
        c = np.ascontiguousarray(connected, np.int32)
        _check(load_library().rsc_kfdb_detect_loop(self.h, int(kf_id), len(i), i, v, len(c), c, float(min_score),
                                                   self._cand, self._n), "rsc_kfdb_detect_loop")
        return self._cand[:self._n[0]].copy()

    def state(self, kf: int):
        """((mnLoopQuery, mnRelocQuery), (mnLoopWords, mnRelocWords), (mLoopScore, mRelocScore))"""
        q = np.zeros(2, np.uint64)
        w = np.zeros(2, np.int32)
        s = np.zeros(2, np.float32)
        _check(load_library().rsc_kfdb_state(self.h, int(kf), q, w, s), "rsc_kfdb_state")
        return tuple(int(x) for x in q), tuple(int(x) for x in w), tuple(float(x) for x in s)

    def close(self):
        if getattr(self, "h", None):
            load_library().rsc_kfdb_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()


class PoseOptResult(C.Structure):
    _fields_ = [("n_good", C.c_int32), ("n_initial", C.c_int32), ("rounds", C.c_int32),
                ("lm_iterations", C.c_int32), ("lm_trials", C.c_int32), ("Tcw", C.c_float * 16)]


_fast = None


def _fast_library():
    """Second handle of librsc.so whose batched reset / iterate prototypes take raw addresses
    (c_void_p) instead of checked ndarrays; used only by SolverBatch with buffers it owns."""
    global _fast
    if _fast is None:
        F = C.CDLL(_lib_path_loaded)
        vp = C.c_void_p
        for kind, rec in (("pnp", PnPResult), ("mlpnp", PnPResult), ("sim3", Sim3Result)):
            f = getattr(F, f"rsc_{kind}_reset_many")
            f.argtypes = [C.POINTER(vp), C.c_int, vp]
            f.restype = C.c_int
            f = getattr(F, f"rsc_{kind}_iterate_many")
            f.argtypes = [C.POINTER(vp), C.c_int, vp, C.POINTER(rec), C.POINTER(vp)]
            f.restype = C.c_int
        _fast = F
    return _fast


_lib_path_loaded = LIB_PATH


def load_library(path: str = LIB_PATH):
    """Load librsc.so (raises if it was not built: no fallback)."""
    global _lib, _lib_path_loaded
    if _lib is not None:
        return _lib
    if not os.path.exists(path):
        raise RuntimeError(f"librsc.so not found at {path}: run __graft_entry__.build() / make")
    L = C.CDLL(path)
    _lib_path_loaded = path
    vp = C.c_void_p
    L.rsc_version.restype = C.c_int
    L.rsc_status_string.restype = C.c_char_p
    L.rsc_status_string.argtypes = [C.c_int]
    L.rsc_context_create.argtypes = [C.c_int, C.POINTER(vp)]
    L.rsc_context_destroy.argtypes = [vp]
    L.rsc_selftest_math.argtypes = [vp, C.c_int, C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_double)]
    L.rsc_context_set_stream.argtypes = [vp, vp]
    L.rsc_context_synchronize.argtypes = [vp]
    L.rsc_context_last_timing.argtypes = [vp, C.POINTER(C.c_double)]
    L.rsc_context_last_kernel_timing.argtypes = [vp, C.POINTER(C.c_double)]
    L.rsc_diag_host_timing.argtypes = [vp, C.POINTER(C.c_double)]
    L.rsc_context_enable_timing.argtypes = [vp, C.c_int]
    L.rsc_context_set_eig_rows.argtypes = [vp, C.c_int]
    L.rsc_context_set_round_args.argtypes = [vp, C.c_int]
    L.rsc_context_set_scan_bound.argtypes = [vp, C.c_int]
    L.rsc_diag_round_paths.argtypes = [vp, C.POINTER(C.c_int64)]
    L.rsc_diag_fill_staging.argtypes = [vp, C.c_int]
    L.rsc_diag_fill_staging.restype = C.c_int64
    L.rsc_diag_localba_stages.argtypes = [vp, C.POINTER(C.c_double), C.c_int]
    L.rsc_local_bundle_adjustment_many.argtypes = [vp, C.POINTER(LocalBAProblem), C.c_int, C.POINTER(LocalBAOut),
                                                   C.POINTER(LocalBAResult)]
    L.rsc_context_set_eig_split.argtypes = [vp, C.c_int]
    L.rsc_context_set_sim3opt_helpers.argtypes = [vp, C.c_int]
    L.rsc_pnp_create.argtypes = [vp, C.POINTER(PnPProblem), C.c_uint32, C.POINTER(vp)]
    L.rsc_pnp_destroy.argtypes = [vp]
    L.rsc_pnp_set_ransac_parameters.argtypes = [vp, C.c_double, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float]
    L.rsc_pnp_iterate.argtypes = [vp, C.c_int, C.POINTER(PnPResult), C.c_void_p]
    L.rsc_pnp_find.argtypes = [vp, C.POINTER(PnPResult), C.c_void_p]
    L.rsc_pnp_last_inliers.argtypes = [vp, C.c_void_p]
    L.rsc_pnp_last_inliers.restype = C.c_int
    L.rsc_pnp_iterate_many.argtypes = [C.POINTER(vp), C.c_int, i32p, C.POINTER(PnPResult), C.POINTER(C.c_void_p)]
    L.rsc_pnp_reset.argtypes = [vp, C.c_uint32]
    L.rsc_pnp_get_state.argtypes = [vp, i32p]
    L.rsc_pnp_last_samples.argtypes = [vp, i32p, C.c_int]
    L.rsc_pnp_last_hypotheses.argtypes = [vp, i32p, f32p, C.c_int]
    L.rsc_pnp_last_counts_raw.argtypes = [vp, i32p, C.c_int]
    L.rsc_sim3_last_hypotheses.argtypes = [vp, i32p, f32p, C.c_int]
    L.rsc_mlpnp_last_counts.argtypes = [vp, i32p, C.c_int]
    L.rsc_sim3_create.argtypes = [vp, C.POINTER(Sim3Input), C.c_uint32, C.POINTER(vp)]
    L.rsc_sim3_destroy.argtypes = [vp]
    L.rsc_sim3_set_ransac_parameters.argtypes = [vp, C.c_double, C.c_int, C.c_int]
    L.rsc_sim3_iterate.argtypes = [vp, C.c_int, C.POINTER(Sim3Result), C.c_void_p]
    L.rsc_sim3_find.argtypes = [vp, C.POINTER(Sim3Result), C.c_void_p]
    L.rsc_sim3_iterate_many.argtypes = [C.POINTER(vp), C.c_int, i32p, C.POINTER(Sim3Result), C.POINTER(C.c_void_p)]
    L.rsc_sim3_reset.argtypes = [vp, C.c_uint32]
    L.rsc_sim3_get_state.argtypes = [vp, i32p]
    L.rsc_sim3_prepared.argtypes = [vp, f32p, f32p, f32p, f32p, u64p, u64p, i32p]
    L.rsc_rand_stream.argtypes = [vp, C.c_uint32, C.c_int, i32p]
    u32p = np.ctypeslib.ndpointer(dtype=np.uint32, flags="C_CONTIGUOUS")
    L.rsc_pnp_reset_many.argtypes = [C.POINTER(vp), C.c_int, u32p]
    L.rsc_pnp_set_ransac_parameters_many.argtypes = [C.POINTER(vp), C.c_int, C.c_double, C.c_int, C.c_int, C.c_int,
                                                     C.c_float, C.c_float]
    L.rsc_sim3_reset_many.argtypes = [C.POINTER(vp), C.c_int, u32p]
    L.rsc_sim3_set_ransac_parameters_many.argtypes = [C.POINTER(vp), C.c_int, C.c_double, C.c_int, C.c_int]
    f64p = np.ctypeslib.ndpointer(dtype=np.float64, flags="C_CONTIGUOUS")
    L.rsc_mlpnp_create.argtypes = [vp, C.POINTER(PnPProblem), C.c_uint32, C.POINTER(vp)]
    L.rsc_mlpnp_destroy.argtypes = [vp]
    L.rsc_mlpnp_set_covariances.argtypes = [vp, C.POINTER(C.c_double)]
    L.rsc_mlpnp_set_ransac_parameters.argtypes = [vp, C.c_double, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float]
    L.rsc_mlpnp_set_ransac_parameters_many.argtypes = [C.POINTER(vp), C.c_int, C.c_double, C.c_int, C.c_int,
                                                       C.c_int, C.c_float, C.c_float]
    L.rsc_mlpnp_iterate.argtypes = [vp, C.c_int, C.POINTER(PnPResult), C.c_void_p]
    L.rsc_mlpnp_iterate_many.argtypes = [C.POINTER(vp), C.c_int, i32p, C.POINTER(PnPResult), C.POINTER(C.c_void_p)]
    L.rsc_mlpnp_reset.argtypes = [vp, C.c_uint32]
    L.rsc_mlpnp_reset_many.argtypes = [C.POINTER(vp), C.c_int, u32p]
    L.rsc_mlpnp_get_state.argtypes = [vp, i32p]
    L.rsc_mlpnp_last_poses.argtypes = [vp, f64p, C.c_int]
    L.rsc_mlpnp_last_samples.argtypes = [vp, i32p, C.c_int]
    L.rsc_reloc_events.argtypes = [C.POINTER(vp), i32p, C.c_int, C.POINTER(PnPResult), C.POINTER(EventResult)]
    L.rsc_stream_create.argtypes = [vp, C.c_uint32, C.POINTER(vp)]
    L.rsc_stream_destroy.argtypes = [vp]
    L.rsc_stream_destroy.restype = None
    L.rsc_stream_skip.argtypes = [vp, C.c_int64]
    L.rsc_stream_position.argtypes = [vp, C.POINTER(C.c_int64)]
    L.rsc_stream_peek.argtypes = [vp, C.c_int, i32p]
    for f in ("rsc_pnp_bind_stream", "rsc_sim3_bind_stream", "rsc_mlpnp_bind_stream"):
        getattr(L, f).argtypes = [vp, vp]
    L.rsc_reloc_events_shared.argtypes = [C.POINTER(vp), i32p, C.c_int, C.POINTER(vp), C.POINTER(PnPResult),
                                          C.POINTER(EventResult)]
    L.rsc_loop_events_shared.argtypes = [C.POINTER(vp), i32p, C.c_int, C.POINTER(vp), C.POINTER(Sim3Result),
                                         C.POINTER(EventResult)]
    L.rsc_pose_optimization_many.argtypes = [vp, C.POINTER(PoseOptProblem), C.c_int, C.POINTER(PoseOptResult),
                                             C.POINTER(C.c_void_p)]
    L.rsc_optimize_sim3_many.argtypes = [vp, C.POINTER(Sim3OptProblem), C.c_int, C.POINTER(Sim3OptResult),
                                         C.POINTER(C.c_void_p)]
    L.rsc_bow_create.argtypes = [vp, C.POINTER(BowFeatures), C.POINTER(vp)]
    L.rsc_bow_destroy.argtypes = [vp]
    L.rsc_bow_set_valid.argtypes = [vp, u8p]
    L.rsc_search_by_bow_frame_many.argtypes = [vp, C.POINTER(vp), C.c_int, vp, C.c_float, C.c_int,
                                               C.POINTER(C.c_void_p), i32p]
    L.rsc_search_by_bow_kf_many.argtypes = [vp, vp, C.POINTER(vp), C.c_int, C.c_float, C.c_int,
                                            C.POINTER(C.c_void_p), i32p]
    L.rsc_diag_bow_phase_stamps.argtypes = [vp, np.ctypeslib.ndpointer(dtype=np.uint64, flags="C_CONTIGUOUS"),
                                            C.c_int]
    L.rsc_diag_refine_phase_stamps.argtypes = [vp, np.ctypeslib.ndpointer(dtype=np.uint64, flags="C_CONTIGUOUS"),
                                               C.c_int]
    L.rsc_diag_solve_phase_stamps.argtypes = [vp, np.ctypeslib.ndpointer(dtype=np.uint64, flags="C_CONTIGUOUS"),
                                              C.c_int]
    L.rsc_diag_mlpnp_phase_stamps.argtypes = [vp, np.ctypeslib.ndpointer(dtype=np.uint64, flags="C_CONTIGUOUS"),
                                              C.c_int]
    L.rsc_diag_poseopt_phases.argtypes = [vp, np.ctypeslib.ndpointer(dtype=np.uint64, flags="C_CONTIGUOUS"), C.c_int]
    L.rsc_diag_sim3opt_phases.argtypes = [vp, np.ctypeslib.ndpointer(dtype=np.uint64, flags="C_CONTIGUOUS"), C.c_int]
    L.rsc_diag_kfdb_stamps.argtypes = [vp, np.ctypeslib.ndpointer(dtype=np.uint64, flags="C_CONTIGUOUS"), C.c_int]
    f32p_ = np.ctypeslib.ndpointer(dtype=np.float32, flags="C_CONTIGUOUS")
    L.rsc_kfview_create.argtypes = [vp, C.POINTER(Sim3KFStruct), C.POINTER(vp)]
    L.rsc_kfview_destroy.argtypes = [vp]
    L.rsc_search_by_sim3_many.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.c_int, f32p_, f32p_, C.c_float,
                                          C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), i32p]
    L.rsc_diag_sim3match_directions.argtypes = [vp, C.c_int, i32p, C.c_int, i32p, C.c_int]
    u32p_ = np.ctypeslib.ndpointer(dtype=np.uint32, flags="C_CONTIGUOUS")
    f64p_ = np.ctypeslib.ndpointer(dtype=np.float64, flags="C_CONTIGUOUS")
    u64p_ = np.ctypeslib.ndpointer(dtype=np.uint64, flags="C_CONTIGUOUS")
    L.rsc_kfdb_create.argtypes = [vp, C.c_uint32, C.c_int, C.c_int, C.POINTER(vp)]
    L.rsc_kfdb_destroy.argtypes = [vp]
    L.rsc_kfdb_add.argtypes = [vp, C.c_int, C.c_int, u32p_, f64p_]
    L.rsc_kfdb_erase.argtypes = [vp, C.c_int]
    L.rsc_kfdb_release.argtypes = [vp, C.c_int]
    L.rsc_kfdb_clear.argtypes = [vp]
    L.rsc_kfdb_set_covisibility.argtypes = [vp, C.c_int, C.c_int, i32p]
    L.rsc_kfdb_set_covisibility_many.argtypes = [vp, C.c_int, i32p, i32p, i32p]
    L.rsc_kfdb_detect_relocalization.argtypes = [vp, C.c_uint64, C.c_int, u32p_, f64p_, i32p, i32p]
    L.rsc_kfdb_detect_loop.argtypes = [vp, C.c_uint64, C.c_int, u32p_, f64p_, C.c_int, i32p, C.c_float, i32p, i32p]
    L.rsc_kfdb_state.argtypes = [vp, C.c_int, u64p_, i32p, f32p_]
    L.rsc_loop_events.argtypes = [C.POINTER(vp), i32p, C.c_int, C.POINTER(Sim3Result), C.POINTER(EventResult)]
    L.rsc_reloc_events_gated.argtypes = [C.POINTER(vp), i32p, C.c_int, C.POINTER(RelocFrame), C.POINTER(PnPResult),
                                         C.POINTER(RelocGateResult), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
    L.rsc_frameview_create.argtypes = [vp, C.POINTER(FrameFeatures), C.POINTER(vp)]
    L.rsc_frameview_destroy.argtypes = [vp]
    L.rsc_kfview_set_angles.argtypes = [vp, f32p_]
    L.rsc_search_by_projection_many.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.c_int, f32p_,
                                                C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_float, C.c_int,
                                                C.c_int, C.POINTER(C.c_void_p), i32p, i32p]
    L.rsc_reloc_refine_many.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.c_int, C.POINTER(RelocFrame),
                                        C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), i32p, f32p_,
                                        C.POINTER(RelocRefineResult)]
    L.rsc_reloc_events_refined.argtypes = [C.POINTER(vp), C.POINTER(RelocCandidate), i32p, C.c_int, C.POINTER(vp),
                                           C.POINTER(RelocFrame), C.POINTER(PnPResult),
                                           C.POINTER(RelocRefinedResult), C.POINTER(C.c_void_p)]
    L.rsc_loop_events_gated.argtypes = [C.POINTER(vp), C.POINTER(LoopCandidate), i32p, C.c_int,
                                        C.POINTER(Sim3Result), C.POINTER(LoopGateResult), C.POINTER(C.c_void_p)]
    L.rsc_mpview_create.argtypes = [vp, C.POINTER(MapPointsStruct), C.POINTER(vp)]
    L.rsc_mpview_destroy.argtypes = [vp]
    L.rsc_search_by_projection_kf_many.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.c_int, f32p_,
                                                   C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_int,
                                                   C.POINTER(C.c_void_p), i32p, i32p]
    L.rsc_fuse_sim3_many.argtypes = [vp, C.POINTER(vp), C.c_int, vp, f32p_, C.POINTER(C.c_void_p), C.c_float,
                                     C.POINTER(C.c_void_p), i32p]
    L.rsc_fuse_kf_many.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.c_int, C.POINTER(C.c_void_p), C.c_float,
                                   C.POINTER(C.c_void_p), i32p]
    L.rsc_update_map_points_many.argtypes = [vp, C.POINTER(vp), C.c_int, C.POINTER(MapPointUpdates), C.c_int,
                                             C.POINTER(MapPointUpdateOut), vp, C.c_void_p]
    L.rsc_mpview_download.argtypes = [vp, u8p, f32p, f32p, f32p, f32p, u8p]
    L.rsc_compute_stereo_matches_many.argtypes = [vp, C.POINTER(vp), C.POINTER(RightFeatures), C.c_int, f32p, f32p,
                                                  C.c_int] + [C.POINTER(C.c_void_p)] * 4 + [C.POINTER(StereoResult)]
    L.rsc_loop_verify_many.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.c_int, f64p_,
                                       C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                       C.POINTER(LoopVerifyResult), C.POINTER(C.c_void_p)]
    L.rsc_frameview_set_stereo.argtypes = [vp, f32p_, C.c_float]
    L.rsc_search_local_points_many.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.c_int, f32p_] + \
        [C.POINTER(C.c_void_p)] * 3 + [C.c_float] * 3 + [C.POINTER(C.c_void_p)] * 2 + [i32p] * 3
    L.rsc_search_by_projection_points_many.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.c_int] + \
        [C.POINTER(C.c_void_p)] * 3 + [C.c_float] * 2 + [C.POINTER(C.c_void_p)] * 2 + [i32p] * 3
    L.rsc_lastframe_create.argtypes = [vp, C.POINTER(LastFrameSlots), C.POINTER(vp)]
    L.rsc_lastframe_destroy.argtypes = [vp]
    L.rsc_lastframe_destroy.restype = None
    L.rsc_search_by_projection_last_many.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.c_int, f32p_, f32p_, f32p_,
                                                     C.POINTER(C.c_void_p), C.c_float, C.c_int,
                                                     C.POINTER(C.c_void_p), i32p, i32p, i32p]
    L.rsc_track_motion_model_many.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.c_int, f32p_, f32p_, f32p_,
                                              C.c_float, i32p, C.POINTER(TrackMotionResult),
                                              C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
    L.rsc_kfview_set_triangulation.argtypes = [vp, C.POINTER(KFTriangulation)]
    L.rsc_search_for_triangulation_many.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp),
                                                    C.c_int, f32p_, C.POINTER(vp), C.POINTER(vp), i32p, C.c_int,
                                                    C.POINTER(vp), i32p, i32p, C.POINTER(vp)]
    L.rsc_triangulate_pairs_many.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.c_int, i32p, C.POINTER(vp),
                                             C.POINTER(vp), C.POINTER(vp)]
    L.rsc_create_new_map_points_many.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.c_int, i32p, C.POINTER(vp),
                                                 C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), i32p]
    L.rsc_voc_create.argtypes = [vp, C.POINTER(VocabularyNodes), C.POINTER(vp)]
    L.rsc_voc_destroy.argtypes = [vp]
    L.rsc_voc_destroy.restype = None
    L.rsc_voc_size.argtypes = [vp, C.POINTER(C.c_uint32)]
    L.rsc_voc_info.argtypes = [vp, i32p]
    L.rsc_voc_transform_many.argtypes = [vp, C.c_int, i32p, C.POINTER(C.c_void_p), C.c_int, C.POINTER(VocOutput)]
    L.rsc_voc_last_kernel_timing.argtypes = [vp, C.POINTER(C.c_double)]
    L.rsc_bow_create_transformed.argtypes = [vp, vp, C.POINTER(BowFeatures), C.c_int, C.POINTER(vp),
                                             C.POINTER(VocOutput)]
    _lib = L
    return L


def _check(st: int, what: str):
    if st != RSC_OK:
        raise RuntimeError(f"rsc: {what}: {load_library().rsc_status_string(st).decode()} ({st})")


class Context:
    """One engine context (HIP stream + work buffers + rand() jump table) on one device."""

    def __init__(self, device: int = 0):
        L = load_library()
        h = C.c_void_p()
        _check(L.rsc_context_create(device, C.byref(h)), "rsc_context_create")
        self.h = h
        self.device = device

    def close(self):
        if getattr(self, "h", None):
            load_library().rsc_context_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def set_stream(self, stream_ptr: int):
        _check(load_library().rsc_context_set_stream(self.h, C.c_void_p(stream_ptr)), "set_stream")

    def synchronize(self):
        _check(load_library().rsc_context_synchronize(self.h), "synchronize")

    def enable_timing(self, on: bool = True):
        _check(load_library().rsc_context_enable_timing(self.h, int(on)), "enable_timing")

    def set_eig_rows(self, max_workgroups: int):
        """Eigen stage in the rows form for launches of <= max_workgroups workgroups (0: off)."""
        _check(load_library().rsc_context_set_eig_rows(self.h, int(max_workgroups)), "set_eig_rows")

    def set_eig_split(self, on: bool):
        """Split-form eigen stage (chase and Q rotations on two waves) for the launches the rows form
        does not take (default on); off: the lane-pair form."""
        _check(load_library().rsc_context_set_eig_split(self.h, int(bool(on))), "set_eig_split")

    def set_round_args(self, on: bool):
        """PnP rounds with their records as kernel arguments and the problem table resident on the
        device (default on); off: every round uploads its descriptor blob."""
        _check(load_library().rsc_context_set_round_args(self.h, int(bool(on))), "set_round_args")

    def set_scan_bound(self, on: bool):
        """PnP scan: stop counting a hypothesis that cannot reach mRansacMinInliers after the first half
        of the point slices (default on); off: every hypothesis is counted in full."""
        _check(load_library().rsc_context_set_scan_bound(self.h, int(bool(on))), "set_scan_bound")

    def round_paths(self):
        """Diagnostic counters of the context's PnP rounds: on the argument path, on the blob path,
        and uploads of the resident problem table."""
        out = (C.c_int64 * 3)()
        _check(load_library().rsc_diag_round_paths(self.h, out), "round_paths")
        return dict(args=int(out[0]), blob=int(out[1]), table_uploads=int(out[2]))

    def fill_staging(self, byte: int) -> int:
        """Diagnostic: fill every staging buffer of the batched calls (device arenas, LM input and result
        buffers, and their pinned mirrors) with `byte` over its whole capacity; returns the bytes filled."""
        n = int(load_library().rsc_diag_fill_staging(self.h, int(byte)))
        if n < 0:
            _check(n, "fill_staging")
        return n

    def set_sim3opt_helpers(self, helpers: int):
        """OptimizeSim3's form: helper workgroups per pair (the cooperative form), 0 = one workgroup
        per pair, -1 = automatic (default)."""
        _check(load_library().rsc_context_set_sim3opt_helpers(self.h, int(helpers)), "set_sim3opt_helpers")

    MATH_FNS = {"sin": 0, "cos": 1, "acos": 2, "cbrt": 3, "log": 4, "logf": 5, "sqrt_unit": 6, "recip_unit": 7,
                "givens_c": 8, "givens_s": 9, "qr_solve": 10, "pow_1_3": 11, "pow_3_2": 12, "rcp_scan": 13,
                "ldlt_lanes": 16}

    def selftest_math(self, fn: str, x):
        """rsc_math.h evaluated on the GPU (f64 array in, f64 array out; logf: float in/out)."""
        x = np.ascontiguousarray(x, np.float64)
        out = np.empty_like(x)
        dp = C.POINTER(C.c_double)
        _check(load_library().rsc_selftest_math(self.h, self.MATH_FNS[fn], x.ctypes.data_as(dp), int(x.size),
                                                out.ctypes.data_as(dp)), "selftest_math")
        return out

    def qr_solve(self, A, b, X0):
        """PnPsolver::qr_solve (the kernels' qr_solve_6x4) ON THE GPU for a batch of 6x4 systems:
        A [k,6,4], b [k,6], X0 [k,4] (kept on the singular bail-out) -> (X [k,4], ok [k] bool)."""
        A = np.asarray(A, np.float64).reshape(-1, 24)
        k = A.shape[0]
        rec = np.zeros((k, 34))
        rec[:, :24] = A
        rec[:, 24:30] = np.asarray(b, np.float64).reshape(k, 6)
        rec[:, 30:34] = np.asarray(X0, np.float64).reshape(k, 4)
        out = self.selftest_math("qr_solve", rec.ravel()).reshape(k, 34)
        return out[:, :4].copy(), out[:, 4] == 1.0

    def last_timing(self):
        out = (C.c_double * 6)()
        _check(load_library().rsc_context_last_kernel_timing(self.h, out), "last_timing")
        return dict(solve_ms=out[0], scan_ms=out[1], refine_ms=out[2], solve_launches=int(out[3]),
                    hypotheses=int(out[4]), eig_ms=out[5])

    def host_timing(self):
        """Diagnostic host clock (us) of the last PnP iterate_many: first launch, enqueued, synced, return."""
        out = (C.c_double * 4)()
        _check(load_library().rsc_diag_host_timing(self.h, out), "host_timing")
        return list(out)

    def rand_stream(self, seed: int, n: int) -> np.ndarray:
        out = np.zeros(n, np.int32)
        _check(load_library().rsc_rand_stream(self.h, seed, n, out), "rand_stream")
        return out


class Stream:
    """The reference's process-global rand() stream (Q3): srand(seed) and a position.  Solvers bound
    to it (``solver.bind_stream(stream)``) draw their samples from it in call order; an event batch
    run with one stream per event (``EventBatch.run(streams=...)``) draws each event's calls from its
    stream in the round-robin's order."""

    def __init__(self, ctx: "Context", seed: int = 1):
        h = C.c_void_p()
        _check(load_library().rsc_stream_create(ctx.h, seed, C.byref(h)), "rsc_stream_create")
        self.h = h
        self.ctx = ctx

    def close(self):
        if getattr(self, "h", None):
            load_library().rsc_stream_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def skip(self, n: int):
        _check(load_library().rsc_stream_skip(self.h, int(n)), "rsc_stream_skip")

    @property
    def position(self) -> int:
        v = C.c_int64()
        _check(load_library().rsc_stream_position(self.h, C.byref(v)), "rsc_stream_position")
        return int(v.value)

    def peek(self, n: int) -> np.ndarray:
        out = np.zeros(max(n, 1), np.int32)
        _check(load_library().rsc_stream_peek(self.h, n, out), "rsc_stream_peek")
        return out[:n]


def _bind(fn, solver, stream):
    _check(fn(solver.h, stream.h if stream is not None else None), "bind_stream")
    solver._stream = stream  # keep the stream alive while bound


def _pnp_out(r: PnPResult, mask) -> dict:
    """Result dict of one PnP / MLPnP iterate().  ``mask`` None = the caller asked for no vbInliers:
    ``inliers`` is then None (never a zero array that reads like a result)."""
    T = np.array(r.T, dtype=np.float32).reshape(4, 4)
    inl = None if mask is None else (mask.astype(bool) if r.ok else np.zeros(0, bool))
    return dict(ok=bool(r.ok), no_more=bool(r.no_more), n_inliers=int(r.n_inliers), iterations=int(r.iterations),
                T=T, inliers=inl)


class PnPSolver:
    """PnPsolver (PnPsolver.cpp) on the GPU.  ``scene`` carries the compacted constructor arrays."""

    def __init__(self, ctx: Context, scene, seed: int = 1):
        L = load_library()
        self.ctx = ctx
        self._keep = [np.ascontiguousarray(scene.p2d, np.float32), np.ascontiguousarray(scene.p3dw, np.float32),
                      np.ascontiguousarray(scene.sigma2, np.float32), np.ascontiguousarray(scene.kp_index, np.int32)]
        pb = PnPProblem(int(scene.n), int(scene.n_points), self._keep[0].ctypes.data, self._keep[1].ctypes.data,
                        self._keep[2].ctypes.data, self._keep[3].ctypes.data, float(scene.fx), float(scene.fy),
                        float(scene.cx), float(scene.cy))
        h = C.c_void_p()
        _check(L.rsc_pnp_create(ctx.h, C.byref(pb), seed, C.byref(h)), "rsc_pnp_create")
        self.h = h
        self.n_points = int(scene.n_points)
        self.n = int(scene.n)

    def close(self):
        if getattr(self, "h", None):
            load_library().rsc_pnp_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def set_ransac_parameters(self, probability=0.99, min_inliers=8, max_iterations=300, min_set=4, epsilon=0.4,
                              th2=5.991):
        _check(load_library().rsc_pnp_set_ransac_parameters(self.h, probability, min_inliers, max_iterations,
                                                            min_set, epsilon, th2), "SetRansacParameters")

    def iterate(self, n_iterations: int) -> dict:
        r = PnPResult()
        mask = np.zeros(max(self.n_points, 1), np.uint8)
        _check(load_library().rsc_pnp_iterate(self.h, n_iterations, C.byref(r), mask.ctypes.data), "iterate")
        return _pnp_out(r, mask[:self.n_points])

    def find(self) -> dict:
        r = PnPResult()
        mask = np.zeros(max(self.n_points, 1), np.uint8)
        _check(load_library().rsc_pnp_find(self.h, C.byref(r), mask.ctypes.data), "find")
        return _pnp_out(r, mask[:self.n_points])

    def last_inliers(self):
        """vbInliers of the last iterate()/find() (bool[n_points]; None when it returned false),
        fetched after the call (rsc_pnp_last_inliers) — e.g. after SolverBatch.iterate_raw."""
        mask = np.zeros(max(self.n_points, 1), np.uint8)
        st = load_library().rsc_pnp_last_inliers(self.h, mask.ctypes.data)
        if st < 0:
            _check(st, "last_inliers")
        return mask[:self.n_points].astype(bool) if st == 1 else None

    def reset(self, seed: int):
        _check(load_library().rsc_pnp_reset(self.h, seed), "reset")

    def bind_stream(self, stream):
        """Draw from a shared Stream (None: back to the own stream) — rsc_pnp_bind_stream."""
        _bind(load_library().rsc_pnp_bind_stream, self, stream)

    def state(self) -> dict:
        out = np.zeros(8, np.int32)
        _check(load_library().rsc_pnp_get_state(self.h, out), "get_state")
        return dict(iterations=int(out[0]), max_iterations=int(out[1]), min_inliers=int(out[2]),
                    best_inliers=int(out[3]), max_rows=int(out[4]), N=int(out[5]), n_points=int(out[6]),
                    min_set=int(out[7]))

    def last_samples(self, cap: int = 100000) -> np.ndarray:
        out = np.zeros((cap, 8), np.int32)
        n = load_library().rsc_pnp_last_samples(self.h, out.reshape(-1), cap)
        return out[:max(n, 0)]

    def last_hypotheses(self, cap: int = 4096):
        """(counts [H], float poses [H, 12] = R row-major + t) of the last launch (parity hook)."""
        cnt = np.zeros(cap, np.int32)
        pos = np.zeros((cap, 12), np.float32)
        n = load_library().rsc_pnp_last_hypotheses(self.h, cnt, pos.reshape(-1), cap)
        if n < 0:
            _check(n, "last_hypotheses")
        return cnt[:n], pos[:n]

    def last_counts_raw(self, cap: int = 4096) -> np.ndarray:
        """The last launch's counts as the round left them: a hypothesis the scan bound cut short shows
        its count over the first segment (before last_hypotheses() has recounted the round)."""
        cnt = np.zeros(cap, np.int32)
        n = load_library().rsc_pnp_last_counts_raw(self.h, cnt, cap)
        if n < 0:
            _check(n, "last_counts_raw")
        return cnt[:n]


def pnp_iterate_many(solvers, n_iterations, with_masks: bool = True):
    """rsc_pnp_iterate_many: iterate() of every solver in one set of launches."""
    L = load_library()
    n = len(solvers)
    hs = (C.c_void_p * n)(*[s.h.value for s in solvers])
    its = np.ascontiguousarray(np.broadcast_to(np.asarray(n_iterations, np.int32), (n,)))
    res = (PnPResult * n)()
    masks = [np.zeros(max(s.n_points, 1), np.uint8) if with_masks else None for s in solvers]
    mp = (C.c_void_p * n)(*[(m.ctypes.data if m is not None else None) for m in masks])
    _check(L.rsc_pnp_iterate_many(hs, n, its, res, mp), "iterate_many")
    return [_pnp_out(res[i], None if masks[i] is None else masks[i][:solvers[i].n_points]) for i in range(n)]


def mlpnp_iterate_many(solvers, n_iterations, with_masks: bool = True):
    """rsc_mlpnp_iterate_many: iterate() of every MLPnP solver in one set of launches."""
    L = load_library()
    n = len(solvers)
    hs = (C.c_void_p * n)(*[s.h.value for s in solvers])
    its = np.ascontiguousarray(np.broadcast_to(np.asarray(n_iterations, np.int32), (n,)))
    res = (PnPResult * n)()
    masks = [np.zeros(max(s.n_points, 1), np.uint8) if with_masks else None for s in solvers]
    mp = (C.c_void_p * n)(*[(m.ctypes.data if m is not None else None) for m in masks])
    _check(L.rsc_mlpnp_iterate_many(hs, n, its, res, mp), "mlpnp_iterate_many")
    return [_pnp_out(res[i], None if masks[i] is None else masks[i][:solvers[i].n_points]) for i in range(n)]


def _sim3_out(r: Sim3Result, mask) -> dict:
    """Result dict of one Sim3 iterate(); ``inliers`` None when no vbInliers were requested."""
    return dict(ok=bool(r.ok), no_more=bool(r.no_more), n_inliers=int(r.n_inliers), iterations=int(r.iterations),
                R=np.array(r.R, np.float32).reshape(3, 3), t=np.array(r.t, np.float32),
                inliers=None if mask is None else mask.astype(bool))


class Sim3Solver:
    """Sim3Solver (Sim3Solver.cpp) on the GPU, built from the raw keyframe-pair inputs."""

    def __init__(self, ctx: Context, pair, seed: int = 1):
        L = load_library()
        self.ctx = ctx
        self._keep = [np.ascontiguousarray(a) for a in (
            pair.valid.astype(np.uint8), pair.Xw1.astype(np.float32), pair.Xw2.astype(np.float32),
            pair.sigma2_1.astype(np.float32), pair.sigma2_2.astype(np.float32))]
        inp = Sim3Input()
        inp.n1 = int(pair.n1)
        inp.valid, inp.Xw1, inp.Xw2, inp.sigma2_1, inp.sigma2_2 = [a.ctypes.data for a in self._keep]
        inp.R1[:] = [float(x) for x in np.asarray(pair.R1, np.float32).ravel()]
        inp.t1[:] = [float(x) for x in np.asarray(pair.t1, np.float32)]
        inp.R2[:] = [float(x) for x in np.asarray(pair.R2, np.float32).ravel()]
        inp.t2[:] = [float(x) for x in np.asarray(pair.t2, np.float32)]
        inp.K1[:] = [float(x) for x in np.asarray(pair.K1, np.float32)]
        inp.K2[:] = [float(x) for x in np.asarray(pair.K2, np.float32)]
        h = C.c_void_p()
        _check(L.rsc_sim3_create(ctx.h, C.byref(inp), seed, C.byref(h)), "rsc_sim3_create")
        self.h = h
        self.n1 = int(pair.n1)

    def close(self):
        if getattr(self, "h", None):
            load_library().rsc_sim3_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def set_ransac_parameters(self, probability=0.99, min_inliers=6, max_iterations=300):
        _check(load_library().rsc_sim3_set_ransac_parameters(self.h, probability, min_inliers, max_iterations),
               "SetRansacParameters")

    def iterate(self, n_iterations: int) -> dict:
        r = Sim3Result()
        mask = np.zeros(max(self.n1, 1), np.uint8)
        _check(load_library().rsc_sim3_iterate(self.h, n_iterations, C.byref(r), mask.ctypes.data), "iterate")
        return _sim3_out(r, mask[:self.n1])

    def find(self) -> dict:
        r = Sim3Result()
        mask = np.zeros(max(self.n1, 1), np.uint8)
        _check(load_library().rsc_sim3_find(self.h, C.byref(r), mask.ctypes.data), "find")
        return _sim3_out(r, mask[:self.n1])

    def reset(self, seed: int):
        _check(load_library().rsc_sim3_reset(self.h, seed), "reset")

    def bind_stream(self, stream):
        _bind(load_library().rsc_sim3_bind_stream, self, stream)

    def state(self) -> dict:
        out = np.zeros(6, np.int32)
        _check(load_library().rsc_sim3_get_state(self.h, out), "get_state")
        return dict(iterations=int(out[0]), max_iterations=int(out[1]), min_inliers=int(out[2]),
                    best_inliers=int(out[3]), N=int(out[4]), n1=int(out[5]))

    def prepared(self) -> dict:
        N = self.state()["N"]
        X1 = np.zeros((N, 3), np.float32); X2 = np.zeros((N, 3), np.float32)
        P1 = np.zeros((N, 2), np.float32); P2 = np.zeros((N, 2), np.float32)
        e1 = np.zeros(N, np.uint64); e2 = np.zeros(N, np.uint64); idx = np.zeros(N, np.int32)
        _check(load_library().rsc_sim3_prepared(self.h, X1, X2, P1, P2, e1, e2, idx), "prepared")
        return dict(X1c=X1, X2c=X2, P1im1=P1, P2im2=P2, maxerr1=e1, maxerr2=e2, indices=idx)

    def last_hypotheses(self, cap: int = 4096):
        """(counts [H], float (R12, t12) [H, 12]) of the last launch (parity hook)."""
        cnt = np.zeros(cap, np.int32)
        pos = np.zeros((cap, 12), np.float32)
        n = load_library().rsc_sim3_last_hypotheses(self.h, cnt, pos.reshape(-1), cap)
        if n < 0:
            _check(n, "last_hypotheses")
        return cnt[:n], pos[:n]


def sim3_iterate_many(solvers, n_iterations, with_masks: bool = True):
    L = load_library()
    n = len(solvers)
    hs = (C.c_void_p * n)(*[s.h.value for s in solvers])
    its = np.ascontiguousarray(np.broadcast_to(np.asarray(n_iterations, np.int32), (n,)))
    res = (Sim3Result * n)()
    masks = [np.zeros(max(s.n1, 1), np.uint8) if with_masks else None for s in solvers]
    mp = (C.c_void_p * n)(*[(m.ctypes.data if m is not None else None) for m in masks])
    _check(L.rsc_sim3_iterate_many(hs, n, its, res, mp), "iterate_many")
    return [_sim3_out(res[i], None if masks[i] is None else masks[i][:solvers[i].n1]) for i in range(n)]


class MLPnPSolver:
    """MLPnPsolver (MLPnPsolver.cpp) on the GPU; same constructor arrays as PnPSolver."""

    def __init__(self, ctx: Context, scene, seed: int = 1):
        L = load_library()
        self.ctx = ctx
        self._keep = [np.ascontiguousarray(scene.p2d, np.float32), np.ascontiguousarray(scene.p3dw, np.float32),
                      np.ascontiguousarray(scene.sigma2, np.float32), np.ascontiguousarray(scene.kp_index, np.int32)]
        pb = PnPProblem(int(scene.n), int(scene.n_points), self._keep[0].ctypes.data, self._keep[1].ctypes.data,
                        self._keep[2].ctypes.data, self._keep[3].ctypes.data, float(scene.fx), float(scene.fy),
                        float(scene.cx), float(scene.cy))
        h = C.c_void_p()
        _check(L.rsc_mlpnp_create(ctx.h, C.byref(pb), seed, C.byref(h)), "rsc_mlpnp_create")
        self.h = h
        self.n_points = int(scene.n_points)
        self.n = int(scene.n)

    def close(self):
        if getattr(self, "h", None):
            load_library().rsc_mlpnp_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def set_covariances(self, cov):
        """computePose's covMats: [n, 3, 3] bearing-vector covariances (None: the reference's path)."""
        if cov is None:
            _check(load_library().rsc_mlpnp_set_covariances(self.h, None), "rsc_mlpnp_set_covariances")
            return
        self._cov = np.ascontiguousarray(np.asarray(cov, np.float64).reshape(self.n, 9))
        _check(load_library().rsc_mlpnp_set_covariances(self.h, self._cov.ctypes.data_as(C.POINTER(C.c_double))),
               "rsc_mlpnp_set_covariances")

    def set_ransac_parameters(self, probability=0.99, min_inliers=8, max_iterations=300, min_set=6, epsilon=0.4,
                              th2=5.991):
        _check(load_library().rsc_mlpnp_set_ransac_parameters(self.h, probability, min_inliers, max_iterations,
                                                              min_set, epsilon, th2), "SetRansacParameters")

    def iterate(self, n_iterations: int) -> dict:
        r = PnPResult()
        mask = np.zeros(max(self.n_points, 1), np.uint8)
        _check(load_library().rsc_mlpnp_iterate(self.h, n_iterations, C.byref(r), mask.ctypes.data), "iterate")
        return _pnp_out(r, mask[:self.n_points])

    def reset(self, seed: int):
        _check(load_library().rsc_mlpnp_reset(self.h, seed), "reset")

    def bind_stream(self, stream):
        _bind(load_library().rsc_mlpnp_bind_stream, self, stream)

    def state(self) -> dict:
        out = np.zeros(6, np.int32)
        _check(load_library().rsc_mlpnp_get_state(self.h, out), "get_state")
        return dict(iterations=int(out[0]), max_iterations=int(out[1]), min_inliers=int(out[2]),
                    best_inliers=int(out[3]), n=int(out[4]), min_set=int(out[5]))

    def last_hypotheses(self, cap=4096):
        """(samples [H, 8], double poses [H, 12]) of the last launch (parity hook)."""
        smp = np.zeros((cap, 8), np.int32)
        pos = np.zeros((cap, 12))
        L = load_library()
        n = L.rsc_mlpnp_last_samples(self.h, smp.reshape(-1), cap)
        m = L.rsc_mlpnp_last_poses(self.h, pos.reshape(-1), cap)
        if n < 0 or m < 0:
            _check(min(n, m), "last_hypotheses")
        if n != m:
            raise RuntimeError(f"last_hypotheses: {n} samples vs {m} poses")
        return smp[:n], pos[:n]

    def last_counts(self, cap=4096):
        cnt = np.zeros(cap, np.int32)
        n = load_library().rsc_mlpnp_last_counts(self.h, cnt, cap)
        if n < 0:
            _check(n, "last_counts")
        return cnt[:n]


class SolverBatch:
    """A fixed list of solvers (one context) with batched reset / SetRansacParameters / iterate —
    the relocalization (PnP) or loop-closure (Sim3) candidate set of one event."""

    def __init__(self, solvers):
        self.solvers = list(solvers)
        first = self.solvers[0]
        self.kind = "pnp" if isinstance(first, PnPSolver) else ("mlpnp" if isinstance(first, MLPnPSolver) else "sim3")
        self._h = (C.c_void_p * len(self.solvers))(*[s.h.value for s in self.solvers])
        n = len(self.solvers)
        # hot-path prototypes with raw addresses (the ndpointer checks cost ~4 us per call): a
        # second handle of the same library keeps the checked prototypes of load_library() intact
        load_library()
        F = _fast_library()
        self._reset_f = {"pnp": F.rsc_pnp_reset_many, "mlpnp": F.rsc_mlpnp_reset_many,
                         "sim3": F.rsc_sim3_reset_many}[self.kind]
        self._iter_f = {"pnp": F.rsc_pnp_iterate_many, "mlpnp": F.rsc_mlpnp_iterate_many,
                        "sim3": F.rsc_sim3_iterate_many}[self.kind]
        self._seeds = np.zeros(n, np.uint32)
        self._seeds_p = self._seeds.ctypes.data
        rec = Sim3Result if self.kind == "sim3" else PnPResult
        self._raw = (rec * n)()
        self._its = np.zeros(n, np.int32)
        self._its_p = self._its.ctypes.data
        self._nomask = (C.c_void_p * n)()
        self._view = np.ctypeslib.as_array(self._raw)

    def reset(self, seeds):
        self._seeds[:] = seeds
        _check(self._reset_f(self._h, len(self.solvers), self._seeds_p), "reset_many")

    def set_ransac_parameters(self, *params):
        L = load_library()
        if self.kind == "pnp":
            _check(L.rsc_pnp_set_ransac_parameters_many(self._h, len(self.solvers), *params), "params_many")
        elif self.kind == "mlpnp":
            _check(L.rsc_mlpnp_set_ransac_parameters_many(self._h, len(self.solvers), *params), "params_many")
        else:
            _check(L.rsc_sim3_set_ransac_parameters_many(self._h, len(self.solvers), *params), "params_many")

    def iterate(self, n_iterations, with_masks=False):
        """iterate() of every solver; ``inliers`` of each result is None unless with_masks."""
        if self.kind == "pnp":
            return pnp_iterate_many(self.solvers, n_iterations, with_masks)
        if self.kind == "mlpnp":
            return mlpnp_iterate_many(self.solvers, n_iterations, with_masks)
        return sim3_iterate_many(self.solvers, n_iterations, with_masks)

    def iterate_raw(self, n_iterations):
        """iterate() of every solver without inlier vectors; returns the C result records as a
        numpy structured array (fields ok, no_more, n_inliers, iterations, T | R, t) without
        per-solver Python objects (the hot loop of bench.py)."""
        self._its[:] = n_iterations
        _check(self._iter_f(self._h, len(self.solvers), self._its_p, self._raw, self._nomask), "iterate_many")
        return self._view


class EventBatch:
    """Config-5 style event driver: many relocalization (PnP) or loop-closure (Sim3) events, each a
    contiguous group of candidate solvers; all candidates of all events run in the same launches
    (rsc_reloc_events / rsc_loop_events)."""

    def __init__(self, events):
        self.events = [list(ev) for ev in events]
        flat = [s for ev in self.events for s in ev]
        self.kind = "sim3" if isinstance(flat[0], Sim3Solver) else "pnp"
        self.batch = SolverBatch(flat)
        self.begin = np.zeros(len(self.events) + 1, np.int32)
        self.begin[1:] = np.cumsum([len(ev) for ev in self.events])
        rec = Sim3Result if self.kind == "sim3" else PnPResult
        self._cand = (rec * len(flat))()
        self._ev = (EventResult * len(self.events))()
        self.cand = np.ctypeslib.as_array(self._cand)
        self.per_event = np.ctypeslib.as_array(self._ev)

    def run(self, streams=None):
        """Run every event.  ``streams``: one Stream per event = the reference's shared rand() stream
        at that event's call (rsc_reloc_events_shared / rsc_loop_events_shared); None = every
        candidate on its own stream (H4)."""
        L = load_library()
        if streams is None:
            f = L.rsc_loop_events if self.kind == "sim3" else L.rsc_reloc_events
            _check(f(self.batch._h, self.begin, len(self.events), self._cand, self._ev), "events")
            return self.per_event
        if len(streams) != len(self.events) or any(st is None for st in streams):
            raise ValueError(f"one Stream per event: {len(self.events)} events, {len(streams)} streams")
        hs = (C.c_void_p * len(streams))(*[st.h.value for st in streams])
        f = L.rsc_loop_events_shared if self.kind == "sim3" else L.rsc_reloc_events_shared
        _check(f(self.batch._h, self.begin, len(self.events), hs, self._cand, self._ev), "events_shared")
        return self.per_event

    def run_reloc_gated(self, frames):
        """Relocalization events with the reference's PoseOptimization gate (rsc_reloc_events_gated,
        Tracking.cpp:1239-1335).  frames[e] = (u_right [n_points] float32 or None, bf).  Returns
        (per-event RelocGateResult records, winner outlier masks, winner vbInliers) — the masks are
        [n_points] uint8 arrays per event (zeros without a winner)."""
        assert self.kind == "pnp"
        if len(frames) != len(self.events):
            raise ValueError(f"one frame per event: {len(self.events)} events, {len(frames)} frames")
        L = load_library()
        fr = (RelocFrame * len(self.events))()
        keep = []
        for e, (ur, bf) in enumerate(frames):
            if ur is not None:
                a = np.ascontiguousarray(ur, np.float32)
                keep.append(a)
                fr[e].u_right = a.ctypes.data
            fr[e].bf = float(bf)
        res = (RelocGateResult * len(self.events))()
        npts = [ev[0].n_points if ev else 0 for ev in self.events]
        outl = [np.zeros(max(n, 1), np.uint8) for n in npts]
        inl = [np.zeros(max(n, 1), np.uint8) for n in npts]
        po = (C.c_void_p * len(self.events))(*[a.ctypes.data for a in outl])
        pi = (C.c_void_p * len(self.events))(*[a.ctypes.data for a in inl])
        _check(L.rsc_reloc_events_gated(self.batch._h, self.begin, len(self.events), fr, self._cand, res, po, pi),
               "reloc_events_gated")
        return np.ctypeslib.as_array(res).copy(), [o[:n] for o, n in zip(outl, npts)], \
            [m[:n] for m, n in zip(inl, npts)]

    def run_reloc_refined(self, views, frames, candidates):
        """Relocalization events from the candidate solvers to bMatch (rsc_reloc_events_refined,
        Tracking.cpp:1239-1335): the gate of run_reloc_gated with the SearchByProjection refinement inside.
        views[e] = FrameView of the event's Frame; frames[e] = (u_right or None, bf); candidates[e][c] =
        (KFView with angles, matches int32 [frame n] = vvpMapPointMatches as KeyFrame slots).  Returns
        (per-event RelocRefinedResult records, the accepted success's mvpMapPoints per event as KeyFrame
        slots of the winner, all -1 without a match)."""
        assert self.kind == "pnp"
        ne = len(self.events)
        if len(frames) != ne or len(views) != ne or len(candidates) != ne or \
                any(len(c) != len(ev) for c, ev in zip(candidates, self.events)):
            raise ValueError("one view and frame per event, one (kf, matches) per candidate")
        L = load_library()
        fr = (RelocFrame * max(ne, 1))()
        keep = []
        for e, (ur, bf) in enumerate(frames):
            if ur is not None:
                a = np.ascontiguousarray(ur, np.float32)
                keep.append(a)
                fr[e].u_right = a.ctypes.data
            fr[e].bf = float(bf)
        flat = [c for cs in candidates for c in cs]
        rc = (RelocCandidate * max(len(flat), 1))()
        for k, (kv, m) in enumerate(flat):
            a = np.ascontiguousarray(m, np.int32)
            keep.append(a)
            rc[k].kf, rc[k].matches = kv.h.value, a.ctypes.data
        res = (RelocRefinedResult * max(ne, 1))()
        mo = [np.full(max(v.n, 1), -1, np.int32) for v in views]
        _check(L.rsc_reloc_events_refined(self.batch._h, rc, self.begin, ne, _handles(views), fr, self._cand, res,
                                          _ptrs(mo)), "reloc_events_refined")
        return np.ctypeslib.as_array(res).copy()[:ne], [m[:v.n] for m, v in zip(mo, views)]

    def run_loop_gated(self, candidates):
        """Loop-closure events with the reference's SearchBySim3 + OptimizeSim3 gate
        (rsc_loop_events_gated, LoopClosing.cpp:268-329).  candidates[e][c] = (KFView of mpCurrentKF,
        KFView of the candidate, matches12 int32 [kf1 n]).  Returns (per-event LoopGateResult records,
        the accepted candidate's mvpCurrentMatchedPoints per event as KF2 indices)."""
        assert self.kind == "sim3"
        if len(candidates) != len(self.events) or any(len(c) != len(ev) for c, ev in zip(candidates, self.events)):
            raise ValueError("one (kf1, kf2, matches12) per candidate of every event")
        L = load_library()
        flat = [c for cs in candidates for c in cs]
        lc = (LoopCandidate * max(len(flat), 1))()
        keep = []
        for k, (v1, v2, m) in enumerate(flat):
            a = np.ascontiguousarray(m, np.int32)
            keep.append(a)
            lc[k].kf1, lc[k].kf2, lc[k].matches12 = v1.h.value, v2.h.value, a.ctypes.data
        res = (LoopGateResult * len(self.events))()
        n1 = [cs[0][0].n if cs else 0 for cs in candidates]
        mo = [np.full(max(n, 1), -1, np.int32) for n in n1]
        pm = (C.c_void_p * len(self.events))(*[a.ctypes.data for a in mo])
        _check(L.rsc_loop_events_gated(self.batch._h, lc, self.begin, len(self.events), self._cand, res, pm),
               "loop_events_gated")
        return np.ctypeslib.as_array(res).copy(), [m[:n] for m, n in zip(mo, n1)]

    def winner_poses(self) -> np.ndarray:
        """[n_events, 16] float32 pose of each event's winning candidate (PnP Tcw row-major, Sim3
        [R|t; 0 0 0 1]); zeros for events without a winner."""
        out = np.zeros((len(self.events), 16), np.float32)
        for e in range(len(self.events)):
            w = int(self.per_event["winner"][e])
            if w < 0:
                continue
            r = self.cand[self.begin[e] + w]
            if self.kind == "pnp":
                out[e] = np.asarray(r["T"], np.float32).ravel()
            else:
                R = np.asarray(r["R"], np.float32).reshape(3, 3)
                out[e, 0:3], out[e, 4:7], out[e, 8:11] = R[0], R[1], R[2]
                out[e, 3], out[e, 7], out[e, 11], out[e, 15] = r["t"][0], r["t"][1], r["t"][2], 1.0
        return out


class PoseOptBatch:
    """Frames prepared once for repeated rsc_pose_optimization_many calls (the ctypes problem
    records and contiguous arrays are built here, so a call is one C entry)."""

    def __init__(self, ctx: Context, frames, with_outliers: bool = True):
        self.ctx = ctx
        self.frames = list(frames)
        n = len(self.frames)
        self.probs = (PoseOptProblem * max(n, 1))()
        self.res = (PoseOptResult * max(n, 1))()
        self.ptrs = (C.c_void_p * max(n, 1))()
        self.keep, self.outs = [], []
        for i, f in enumerate(self.frames):
            arrs = [np.ascontiguousarray(f.has_mp, np.uint8), np.ascontiguousarray(f.uv, np.float32).reshape(-1),
                    np.ascontiguousarray(f.Xw, np.float32).reshape(-1),
                    np.ascontiguousarray(f.inv_sigma2, np.float32)]
            ur = getattr(f, "u_right", None)
            if ur is not None:
                arrs.append(np.ascontiguousarray(ur, np.float32))
            self.keep.append(arrs)
            p = self.probs[i]
            p.n = f.n
            p.has_mp, p.uv, p.Xw, p.inv_sigma2 = (a.ctypes.data for a in arrs[:4])
            p.u_right = arrs[4].ctypes.data if ur is not None else None
            p.bf = float(getattr(f, "bf", 0.0))
            p.fx, p.fy, p.cx, p.cy = float(f.fx), float(f.fy), float(f.cx), float(f.cy)
            p.Tcw[:] = [float(v) for v in np.asarray(f.Tcw, np.float32).reshape(16)]
            o = np.full(max(f.n, 1), 255, np.uint8)
            self.outs.append(o)
            self.ptrs[i] = o.ctypes.data if with_outliers else None

    def run(self):
        _check(load_library().rsc_pose_optimization_many(self.ctx.h, self.probs, len(self.frames), self.res,
                                                         self.ptrs), "rsc_pose_optimization_many")

    def results(self):
        out = []
        for i, f in enumerate(self.frames):
            r = self.res[i]
            out.append({"n_good": r.n_good, "n_initial": r.n_initial, "rounds": r.rounds,
                        "lm_iterations": r.lm_iterations, "lm_trials": r.lm_trials,
                        "Tcw": np.array(r.Tcw[:], np.float32).reshape(4, 4), "outlier": self.outs[i][:f.n].copy()})
        return out


class Sim3OptBatch:
    """Loop-closure pairs prepared once for repeated rsc_optimize_sim3_many calls
    (Optimizer::OptimizeSim3, Optimizer.cpp:1054-1250).  problems: rsc.synth.Sim3OptProblem-likes."""

    def __init__(self, ctx: Context, problems):
        self.ctx = ctx
        self.problems = list(problems)
        n = len(self.problems)
        self.probs = (Sim3OptProblem * max(n, 1))()
        self.res = (Sim3OptResult * max(n, 1))()
        self.ptrs = (C.c_void_p * max(n, 1))()
        self.keep, self.keeps = [], []
        for i, p in enumerate(self.problems):
            arrs = [np.ascontiguousarray(p.valid, np.uint8)] + [np.ascontiguousarray(a, np.float32).reshape(-1) for a in
                                                                (p.X1w, p.X2w, p.uv1, p.uv2, p.inv1, p.inv2)]
            self.keep.append(arrs)
            q = self.probs[i]
            q.n = p.n
            q.valid, q.X1w, q.X2w, q.uv1, q.uv2, q.inv1, q.inv2 = (a.ctypes.data for a in arrs)
            q.R1w[:] = [float(v) for v in np.asarray(p.R1w, np.float32).ravel()]
            q.t1w[:] = [float(v) for v in np.asarray(p.t1w, np.float32)]
            q.R2w[:] = [float(v) for v in np.asarray(p.R2w, np.float32).ravel()]
            q.t2w[:] = [float(v) for v in np.asarray(p.t2w, np.float32)]
            q.K1[:] = [float(v) for v in np.asarray(p.K1, np.float32)]
            q.K2[:] = [float(v) for v in np.asarray(p.K2, np.float32)]
            q.S[:] = [float(v) for v in np.asarray(p.S0, np.float64)]
            q.th2 = float(p.th2)
            k = np.full(max(p.n, 1), 7, np.uint8)
            self.keeps.append(k)
            self.ptrs[i] = k.ctypes.data

    def run(self):
        _check(load_library().rsc_optimize_sim3_many(self.ctx.h, self.probs, len(self.problems), self.res, self.ptrs),
               "rsc_optimize_sim3_many")

    def results(self):
        out = []
        for i, p in enumerate(self.problems):
            r = self.res[i]
            out.append({"n_inliers": r.n_inliers, "n_correspondences": r.n_correspondences, "n_bad": r.n_bad,
                        "lm_iterations": r.lm_iterations, "lm_trials": r.lm_trials,
                        "S": np.array(r.S[:], np.float64), "keep": self.keeps[i][:p.n].copy()})
        return out


def optimize_sim3_many(ctx: Context, problems):
    """Optimizer::OptimizeSim3 on every loop-closure pair in one launch.  Returns per pair a dict:
    n_inliers (the reference's return value), n_correspondences, n_bad, lm_iterations, lm_trials,
    S float64[8] (g2oS12 after the call: q x, y, z, w, t, s), keep uint8[n] (0 where vpMatches1[i]
    is set to NULL)."""
    b = Sim3OptBatch(ctx, problems)
    b.run()
    return b.results()


def pose_optimization_many(ctx: Context, frames, with_outliers: bool = True):
    """Optimizer::PoseOptimization (src/Optimizer.cpp:205-424) on every frame in one launch.

    frames: objects with has_mp, uv, Xw, inv_sigma2, Tcw, fx..cy and optionally u_right (mvuRight,
    >= 0 on stereo slots) + bf (rsc.synth.PoseOptFrame).  Returns
    per frame a dict: n_good (the reference's return value), n_initial, rounds, lm_iterations,
    lm_trials, Tcw float32[4,4] (pFrame->mTcw after the call), outlier uint8[n] (mvbOutlier; 255 on
    slots without a map point)."""
    b = PoseOptBatch(ctx, frames, with_outliers)
    b.run()
    return b.results()


class BowView:
    """A KeyFrame's / Frame's ORB features resident in HBM for ORBmatcher::SearchByBoW: descriptors
    (mDescriptors), keypoint angles, map-point validity and the DBoW2 FeatureVector (mFeatVec) as
    CSR (rsc_bow_features, include/rsc.h).  `view` is an object with n, desc uint8[n,32],
    angle float32[n], valid uint8[n] (or None), node_id uint32[], node_begin int32[], feat uint32[]
    (rsc.synth.BowFeatures)."""

    def __init__(self, ctx: Context, view):
        self.ctx = ctx
        self.n = int(view.n)
        arrs = [np.ascontiguousarray(view.desc, np.uint8).reshape(-1), np.ascontiguousarray(view.angle, np.float32),
                None if view.valid is None else np.ascontiguousarray(view.valid, np.uint8),
                np.ascontiguousarray(view.node_id, np.uint32), np.ascontiguousarray(view.node_begin, np.int32),
                np.ascontiguousarray(view.feat, np.uint32)]
        f = BowFeatures()
        f.n = self.n
        f.desc, f.angle = arrs[0].ctypes.data, arrs[1].ctypes.data
        f.valid = None if arrs[2] is None else arrs[2].ctypes.data
        f.n_nodes = len(arrs[3])
        f.node_id, f.node_begin, f.feat = arrs[3].ctypes.data, arrs[4].ctypes.data, arrs[5].ctypes.data
        h = C.c_void_p()
        _check(load_library().rsc_bow_create(ctx.h, C.byref(f), C.byref(h)), "rsc_bow_create")
        self.h = h

    @classmethod
    def from_descriptors(cls, ctx: Context, voc, desc, angle, valid=None, levelsup: int = 4):
        """A BowView whose FeatureVector the vocabulary computes on the device
        (rsc_bow_create_transformed).  The view's BowVector is left in .word_id / .word_value (for
        KeyFrameDatabase.add / detect_*)."""
        self = cls.__new__(cls)
        self.ctx = ctx
        d = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        self.n = len(d)
        a = np.ascontiguousarray(angle, np.float32)
        v = None if valid is None else np.ascontiguousarray(valid, np.uint8)
        f = BowFeatures()
        f.n = self.n
        f.desc, f.angle = d.ctypes.data, a.ctypes.data
        f.valid = None if v is None else v.ctypes.data
        buf = _VocBuffers(self.n, per_feature=False, feature_vector=False)
        o = VocOutput()
        buf.fill(o)
        h = C.c_void_p()
        _check(load_library().rsc_bow_create_transformed(ctx.h, voc.h, C.byref(f), int(levelsup), C.byref(h), C.byref(o)),
               "rsc_bow_create_transformed")
        self.h = h
        r = buf.result(o)
        self.word_id, self.word_value = r["word_id"], r["word_value"]
        return self

    def set_valid(self, valid):
        _check(load_library().rsc_bow_set_valid(self.h, np.ascontiguousarray(valid, np.uint8)), "rsc_bow_set_valid")

    def close(self):
        if getattr(self, "h", None):
            load_library().rsc_bow_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()


class BowSearch:
    """Prepared SearchByBoW batch (ORBmatcher.cpp:110-240 / :354-488): `count` searches in one launch.

    frame_overload=True: SearchByBoW(pKF = others[c], F = shared) -> rows of shared.n (KeyFrame index
    per Frame feature).  False: SearchByBoW(pKF1 = shared, pKF2 = others[c]) -> rows of shared.n
    (KF2 index per KF1 feature)."""

    def __init__(self, ctx: Context, shared: BowView, others, frame_overload: bool, nnratio: float = 0.75,
                 check_orientation: bool = True):
        self.ctx, self.shared, self.others = ctx, shared, list(others)
        self.frame_overload = frame_overload
        self.nnratio, self.check = float(nnratio), int(bool(check_orientation))
        c = len(self.others)
        self.handles = (C.c_void_p * max(c, 1))(*[o.h for o in self.others])
        self.out = np.zeros((max(c, 1), max(shared.n, 1)), np.int32)
        self.ptrs = (C.c_void_p * max(c, 1))(*[self.out[i].ctypes.data for i in range(c)])
        self.nmatches = np.zeros(max(c, 1), np.int32)

    def run(self):
        L = load_library()
        c = len(self.others)
        if self.frame_overload:
            st = L.rsc_search_by_bow_frame_many(self.ctx.h, self.handles, c, self.shared.h, self.nnratio, self.check,
                                                self.ptrs, self.nmatches)
        else:
            st = L.rsc_search_by_bow_kf_many(self.ctx.h, self.shared.h, self.handles, c, self.nnratio, self.check,
                                             self.ptrs, self.nmatches)
        _check(st, "rsc_search_by_bow")
        c = len(self.others)
        return self.out[:c, :self.shared.n], self.nmatches[:c]


def search_by_bow_frame_many(ctx: Context, kfs, frame, nnratio=0.75, check_orientation=True):
    """SearchByBoW(pKF, F, vpMapPointMatches) for every KeyFrame view against one Frame view
    (Tracking::Relocalization, Tracking.cpp:1207-1214: ORBmatcher(0.75, true)).  Returns
    (matches int32[count, F.n] = KeyFrame feature index or -1, nmatches int32[count])."""
    return BowSearch(ctx, frame, kfs, True, nnratio, check_orientation).run()


def search_by_bow_kf_many(ctx: Context, kf1, kf2s, nnratio=0.75, check_orientation=True):
    """SearchByBoW(pKF1, pKF2, vpMatches12) of one KeyFrame view against each candidate
    (LoopClosing::ComputeSim3, LoopClosing.cpp:238-251).  Returns (matches12 int32[count, kf1.n],
    nmatches int32[count])."""
    return BowSearch(ctx, kf1, kf2s, False, nnratio, check_orientation).run()


class _VocBuffers:
    """Host arrays behind one rsc_voc_output (room for n entries each)."""

    def __init__(self, n: int, per_feature: bool = True, feature_vector: bool = True):
        m = max(int(n), 1)
        self.n = int(n)
        self.word_id, self.word_value = np.zeros(m, np.uint32), np.zeros(m, np.float64)
        self.node_id, self.node_begin = np.zeros(m, np.uint32), np.zeros(m + 1, np.int32)
        self.feat = np.zeros(m, np.uint32)
        self.f_word, self.f_node, self.f_stopped = np.zeros(m, np.uint32), np.zeros(m, np.uint32), np.zeros(m, np.uint8)
        self.per_feature, self.feature_vector = per_feature, feature_vector

    def fill(self, o: VocOutput):
        o.word_id, o.word_value = self.word_id.ctypes.data, self.word_value.ctypes.data
        if self.feature_vector:
            o.node_id, o.node_begin, o.feat = self.node_id.ctypes.data, self.node_begin.ctypes.data, self.feat.ctypes.data
        if self.per_feature:
            o.feature_word, o.feature_node = self.f_word.ctypes.data, self.f_node.ctypes.data
            o.feature_stopped = self.f_stopped.ctypes.data

    def result(self, o: VocOutput) -> dict:
        nw, nn = int(o.n_words), int(o.n_nodes)
        r = dict(word_id=self.word_id[:nw].copy(), word_value=self.word_value[:nw].copy())
        if self.feature_vector:
            begin = self.node_begin[:nn + 1].copy()
            r.update(node_id=self.node_id[:nn].copy(), node_begin=begin, feat=self.feat[:int(begin[nn])].copy())
        if self.per_feature:
            r.update(f_word=self.f_word[:self.n].copy(), f_node=self.f_node[:self.n].copy(),
                     f_stopped=self.f_stopped[:self.n].copy())
        return r


class Vocabulary:
    """The ORB vocabulary resident in HBM (rsc_voc_*): DBoW2 TemplatedVocabulary::transform, i.e.
    Frame::ComputeBoW / KeyFrame::ComputeBoW, on the device.  `nodes` is an object with k, L, scoring,
    weighting, parent int32[], is_leaf uint8[], desc uint8[,32], weight float64[] (rsc.synth.Vocabulary).
    lds_budget_bytes: test hook of the LDS staging cut (0 = default)."""

    def __init__(self, ctx: Context, nodes, lds_budget_bytes: int = 0):
        self.ctx = ctx
        arrs = [np.ascontiguousarray(nodes.parent, np.int32), np.ascontiguousarray(nodes.is_leaf, np.uint8),
                np.ascontiguousarray(nodes.desc, np.uint8).reshape(-1), np.ascontiguousarray(nodes.weight, np.float64)]
        v = VocabularyNodes()
        v.k, v.L, v.scoring, v.weighting = int(nodes.k), int(nodes.L), int(nodes.scoring), int(nodes.weighting)
        v.n_nodes = len(arrs[0])
        v.parent, v.is_leaf, v.desc, v.weight = (a.ctypes.data for a in arrs)
        v.lds_budget_bytes = int(lds_budget_bytes)
        h = C.c_void_p()
        _check(load_library().rsc_voc_create(ctx.h, C.byref(v), C.byref(h)), "rsc_voc_create")
        self.h = h
        n = C.c_uint32()
        _check(load_library().rsc_voc_size(self.h, C.byref(n)), "rsc_voc_size")
        self.size = int(n.value)

    def info(self) -> dict:
        a = np.zeros(8, np.int32)
        _check(load_library().rsc_voc_info(self.h, a), "rsc_voc_info")
        return dict(lds_nodes=int(a[0]), lds_levels=int(a[1]), min_leaf_depth=int(a[2]), max_depth=int(a[3]),
                    max_children=int(a[4]))

    def transform_many(self, descs, levelsup: int = 4, per_feature: bool = True):
        """transform() of every view of `descs` (uint8 [n,32] each) in one call -> a list of dicts:
        word_id uint32[], word_value float64[] (BowVector), node_id uint32[], node_begin int32[],
        feat uint32[] (FeatureVector as CSR) and, with per_feature, f_word / f_node / f_stopped [n]."""
        ds = [np.ascontiguousarray(d, np.uint8).reshape(-1, 32) for d in descs]
        c = len(ds)
        n = np.array([len(d) for d in ds] + [0], np.int32)
        ptrs = (C.c_void_p * max(c, 1))(*[d.ctypes.data for d in ds])
        outs = (VocOutput * max(c, 1))()
        bufs = [_VocBuffers(len(d), per_feature) for d in ds]
        for b, o in zip(bufs, outs):
            b.fill(o)
        _check(load_library().rsc_voc_transform_many(self.h, c, n, ptrs, int(levelsup), outs), "rsc_voc_transform_many")
        return [b.result(o) for b, o in zip(bufs, outs)]

    def transform(self, desc, levelsup: int = 4) -> dict:
        return self.transform_many([desc], levelsup)[0]

    def last_kernel_timing(self):
        """(descent, build) device milliseconds of the last transform (Context.enable_timing)."""
        ms = (C.c_double * 2)()
        _check(load_library().rsc_voc_last_kernel_timing(self.h, ms), "rsc_voc_last_kernel_timing")
        return float(ms[0]), float(ms[1])

    def close(self):
        if getattr(self, "h", None):
            load_library().rsc_voc_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()
