// rsc_views.cpp — the resident views of the C ABI: create / destroy / set_* of rsc_kfview, rsc_frameview,
// rsc_mpview, rsc_lastframe and rsc_bow, with their argument checks.
#include <cmath>
#include <cstring>
#include <memory>
#include "rsc_host.h"

extern "C" {

namespace {
int check_sim3_kf(const rsc_sim3_kf& k) {
    if (k.n < 0 || k.n_levels < 1 || !k.cell_begin || !k.scale_factors) return RSC_ERR_ARG;
    if (k.n > 0 && (!k.kp || !k.octave || !k.desc || !k.mp_state || !k.mp_pos || !k.mp_dmax || !k.mp_dmin ||
                    !k.mp_desc))
        return RSC_ERR_ARG;
    if (int e = check_grid_csr(k.cell_begin, k.cell_feat, kSim3GridCols * kSim3GridRows, k.n, g_last_error)) return e;
    // PredictScale converts ceil(log(mfMaxDistance / dist) / mfLogScaleFactor) to int: out of int's range
    // (undefined) for a non-finite distance bound, so a good MapPoint must carry finite ones
    for (int i = 0; i < k.n; ++i)
        if (k.mp_state[i] == 1 && !(std::isfinite(k.mp_dmax[i]) && std::isfinite(k.mp_dmin[i]))) {
            g_last_error = "non-finite mfMaxDistance / mfMinDistance of a good MapPoint";
            return RSC_ERR_ARG;
        }
    return 0;
}

// the side uploads of a view (rsc_kfview_set_angles, rsc_frameview_set_stereo): n floats, an allocation even for n == 0
static int upload_floats(rsc_context* C, DevBuf<float>& buf, const float* src, int n) {
    RSC_HIP(hipSetDevice(C->device));
    if (int e = buf.ensure((size_t)std::max(n, 1))) return e;
    RSC_HIP(hipStreamSynchronize(C->stream));
    if (n) RSC_HIP(hipMemcpy(buf.p, src, 4 * (size_t)n, hipMemcpyHostToDevice));
    return 0;
}
}  // namespace

// the validity flags of a FeatureVector's host copy (rsc_bow::feat), re-applied
void flag_invalid(std::vector<uint32_t>& feat, const uint8_t* valid) {
    for (uint32_t& x : feat) {
        x &= ~kBowInvalid;
        if (valid && !valid[x]) x |= kBowInvalid;
    }
}

// ---- ORBmatcher::SearchByBoW (src/ORBmatcher.cpp:110-240, :354-488) ----
int rsc_bow_create(rsc_context* C, const rsc_bow_features* f, rsc_bow** out) {
    if (!C || !f || !out) return RSC_ERR_ARG;
    *out = nullptr;
    const int n = f->n, nn = f->n_nodes;
    if (n < 0 || nn < 0 || (n > 0 && (!f->desc || !f->angle)) || (nn > 0 && (!f->node_id || !f->node_begin || !f->feat)))
        return RSC_ERR_ARG;
    if (n > kBowMaxFeatures || nn > kBowMaxFeatures) {
        g_last_error = "more than 8192 keypoints (or FeatureVector nodes) in one view";
        return RSC_ERR_UNSUPPORTED;
    }
    // FeatureVector invariants the node-parallel walk relies on (DBoW2 transform guarantees them)
    const int nf = nn ? f->node_begin[nn] : 0;
    if (nn && f->node_begin[0] != 0) return RSC_ERR_ARG;
    std::vector<uint8_t> seen((size_t)n, 0);
    for (int k = 0; k < nn; ++k) {
        if (f->node_begin[k + 1] < f->node_begin[k]) return RSC_ERR_ARG;
        if (k && f->node_id[k] <= f->node_id[k - 1]) {
            g_last_error = "FeatureVector node ids must be strictly ascending";
            return RSC_ERR_ARG;
        }
    }
    for (int i = 0; i < nf; ++i) {
        const uint32_t x = f->feat[i];
        if (x >= (uint32_t)n || seen[x]) {
            g_last_error = "FeatureVector feature index out of range or repeated";
            return RSC_ERR_ARG;
        }
        seen[x] = 1;
    }
    std::unique_ptr<rsc_bow> b(new rsc_bow);
    b->ctx = C;
    b->n = n;
    b->n_nodes = nn;
    b->n_feat = nf;
    b->feat.assign(f->feat, f->feat + nf);
    flag_invalid(b->feat, f->valid);
    DevBow& hd = b->hdr;
    hd.n = n;
    hd.n_nodes = nn;
    ViewImage img(36 * ((size_t)n + nf) + 8 * (size_t)nn + 7 * 256);  // the six pieces and their padding
    img.put(hd.desc, f->desc, 2 * (size_t)n);                  // a descriptor is two uint4
    const auto dfv = img.hold(hd.desc_fv, 2 * (size_t)nf);     // the descriptors in FeatureVector order
    img.put(hd.angle, f->angle, (size_t)n);
    img.put(hd.node_id, f->node_id, (size_t)nn);
    const auto beg = img.hold(hd.node_begin, (size_t)nn + 1);  // one zero entry without nodes
    const auto feat = img.put(hd.feat, b->feat.data(), (size_t)nf);
    for (int e = 0; e < nf; ++e) std::memcpy(at(img.h.data(), dfv) + 2 * e, f->desc + 32 * (size_t)f->feat[e], 32);
    if (nn) std::memcpy(at(img.h.data(), beg), f->node_begin, 4 * ((size_t)nn + 1));
    if (int e = upload_image(C, b->mem, img)) return e;
    b->off_feat = feat.off;
    *out = b.release();
    return RSC_OK;
}

void rsc_bow_destroy(rsc_bow* b) { destroy_on_stream(b); }

int rsc_bow_set_valid(rsc_bow* b, const uint8_t* valid) {
    if (!b || (b->n && !valid)) return RSC_ERR_ARG;
    if (!b->n_feat) return RSC_OK;
    flag_invalid(b->feat, valid);
    RSC_HIP(hipStreamSynchronize(b->ctx->stream));
    RSC_HIP(hipMemcpy(b->mem.p + b->off_feat, b->feat.data(), 4 * (size_t)b->n_feat, hipMemcpyHostToDevice));
    return RSC_OK;
}

// ---- ORBmatcher::SearchBySim3 (src/ORBmatcher.cpp:948-1170) ----
int rsc_kfview_create(rsc_context* C, const rsc_sim3_kf* k, rsc_kfview** out) {
    if (!C || !k || !out) return RSC_ERR_ARG;
    *out = nullptr;
    if (int e = check_sim3_kf(*k)) return e;
    const int cells = kSim3GridCols * kSim3GridRows;
    const size_t n = (size_t)k->n, nf = (size_t)k->cell_begin[cells];
    std::unique_ptr<rsc_kfview> v(new rsc_kfview);
    v->ctx = C;
    v->n = k->n;
    DevSim3KF& h = v->dev;
    ViewImage img;
    const auto hdr = img.hold(v->hdr, 1);
    img.put(h.kp, k->kp, n);
    img.put(h.octave, k->octave, n);
    img.put(h.desc, k->desc, 2 * n);  // a descriptor is two uint4
    img.put(h.cell_begin, k->cell_begin, (size_t)(cells + 1));
    img.put(h.cell_feat, k->cell_feat, nf);
    img.put(h.scale, k->scale_factors, (size_t)k->n_levels);
    img.put(h.mp_state, k->mp_state, n);
    img.put(h.mp_pos, k->mp_pos, 3 * n);
    img.put(h.mp_dmax, k->mp_dmax, n);
    img.put(h.mp_dmin, k->mp_dmin, n);
    img.put(h.mp_desc, k->mp_desc, 2 * n);
    h.min_x = k->min_x; h.max_x = k->max_x; h.min_y = k->min_y; h.max_y = k->max_y;
    h.gw_inv = k->grid_w_inv; h.gh_inv = k->grid_h_inv;
    h.fx = k->fx; h.fy = k->fy; h.cx = k->cx; h.cy = k->cy;
    h.log_sf = k->log_scale_factor;
    std::memcpy(h.R, k->Rcw, sizeof(h.R));
    std::memcpy(h.t, k->tcw, sizeof(h.t));
    h.n = k->n;
    h.n_levels = k->n_levels;
    if (int e = upload_image(C, v->mem, img, false, hdr, &h)) return e;
    v->kfp = DevKfpKF(reinterpret_cast<const ProjPt*>(h.kp), h.octave, reinterpret_cast<const ProjDesc*>(h.desc),
                      h.cell_begin, h.cell_feat, h.scale, h.min_x, h.max_x, h.min_y, h.max_y, h.gw_inv, h.gh_inv, h.fx,
                      h.fy, h.cx, h.cy, h.log_sf, h.n, h.n_levels);
    v->proj = DevProjKF{h.mp_state, h.mp_pos, h.mp_dmax, h.mp_dmin, reinterpret_cast<const ProjDesc*>(h.mp_desc),
                        nullptr, k->n};
    v->octaves_ok = std::all_of(k->octave, k->octave + n, [&](int32_t o) { return o >= 0 && o < k->n_levels; });
    v->kp.assign(k->kp, k->kp + 2 * n);
    v->octave.assign(k->octave, k->octave + n);
    v->mp_state.assign(k->mp_state, k->mp_state + n);
    v->mp_pos.assign(k->mp_pos, k->mp_pos + 3 * n);
    // mvLevelSigma2[l] = mvScaleFactor[l]^2, mvInvLevelSigma2[l] = 1.0f / mvLevelSigma2[l] (float,
    // ORBextractor's constructor; KeyFrame copies them from the Frame)
    v->inv_level_sigma2.resize((size_t)k->n_levels);
    for (int l = 0; l < k->n_levels; ++l) {
        const float s2 = k->scale_factors[l] * k->scale_factors[l];
        v->inv_level_sigma2[l] = 1.0f / s2;
    }
    std::memcpy(v->R, k->Rcw, sizeof(v->R));
    std::memcpy(v->t, k->tcw, sizeof(v->t));
    v->K[0] = k->fx; v->K[1] = k->fy; v->K[2] = k->cx; v->K[3] = k->cy;
    v->top_scale = k->scale_factors[k->n_levels - 1];
    *out = v.release();
    return RSC_OK;
}

void rsc_kfview_destroy(rsc_kfview* v) { destroy_on_stream(v); }

// ---- ORBmatcher::SearchByProjection(Frame&, KeyFrame, sAlreadyFound, th, ORBdist) (rsc_frameproj.h) ----
int rsc_frameview_create(rsc_context* C, const rsc_frame_features* f, rsc_frameview** out) {
    if (!C || !f || !out) return RSC_ERR_ARG;
    *out = nullptr;
    if (f->n < 0 || f->n > kProjMaxFeatures || f->n_levels < 1 || f->n_levels > 64 || !f->cell_begin ||
        !f->scale_factors)
        return RSC_ERR_ARG;
    if (f->n > 0 && (!f->kp || !f->octave || !f->angle || !f->desc)) return RSC_ERR_ARG;
    const int cells = kProjGridCols * kProjGridRows;
    if (int e = check_grid_csr(f->cell_begin, f->cell_feat, cells, f->n, g_last_error)) return e;
    const size_t n = (size_t)f->n, nf = (size_t)f->cell_begin[cells];
    for (size_t i = 0; i < n; ++i)
        if (f->octave[i] < 0 || f->octave[i] >= f->n_levels) {
            g_last_error = "keypoint octave out of range";
            return RSC_ERR_ARG;
        }
    std::unique_ptr<rsc_frameview> v(new rsc_frameview);
    v->ctx = C;
    v->n = f->n;
    DevProjFrame h;
    ViewImage img;
    const auto hdr = img.hold(v->hdr, 1);
    img.put(h.kp, f->kp, n);
    img.put(h.octave, f->octave, n);
    img.put(h.angle, f->angle, n);
    img.put(h.desc, f->desc, n);
    img.put(h.cell_begin, f->cell_begin, (size_t)(cells + 1));
    img.put(h.cell_feat, f->cell_feat, nf);
    img.put(h.scale, f->scale_factors, (size_t)f->n_levels);
    h.min_x = f->min_x; h.max_x = f->max_x; h.min_y = f->min_y; h.max_y = f->max_y;
    h.gw_inv = f->grid_w_inv; h.gh_inv = f->grid_h_inv;
    h.fx = f->fx; h.fy = f->fy; h.cx = f->cx; h.cy = f->cy;
    h.log_sf = f->log_scale_factor;
    h.n = f->n;
    h.n_levels = f->n_levels;
    if (int e = upload_image(C, v->mem, img, false, hdr, &h)) return e;
    v->kp.assign(f->kp, f->kp + 2 * n);
    v->octave.assign(f->octave, f->octave + n);
    v->inv_level_sigma2.resize((size_t)f->n_levels);
    for (int l = 0; l < f->n_levels; ++l) {  // mvInvLevelSigma2 as ORBextractor sets it (see rsc_kfview_create)
        const float s2 = f->scale_factors[l] * f->scale_factors[l];
        v->inv_level_sigma2[l] = 1.0f / s2;
    }
    v->K[0] = f->fx; v->K[1] = f->fy; v->K[2] = f->cx; v->K[3] = f->cy;
    v->top_scale = f->scale_factors[f->n_levels - 1];
    v->gw_inv = f->grid_w_inv;
    v->gh_inv = f->grid_h_inv;
    *out = v.release();
    return RSC_OK;
}

void rsc_frameview_destroy(rsc_frameview* v) { destroy_on_stream(v); }

int rsc_kfview_set_angles(rsc_kfview* v, const float* angle) {
    if (!v || (v->n > 0 && !angle)) return RSC_ERR_ARG;
    if (int e = upload_floats(v->ctx, v->d_angle, angle, v->n)) return e;
    v->proj.angle = v->d_angle.p;
    v->has_angles = true;
    return RSC_OK;
}

int rsc_frameview_set_stereo(rsc_frameview* v, const float* u_right, float mbf) {
    if (!v || (v->n > 0 && !u_right)) return RSC_ERR_ARG;
    if (int e = upload_floats(v->ctx, v->d_uright, u_right, v->n)) return e;
    v->h_uright.assign(u_right, u_right + (v->n > 0 ? v->n : 0));
    v->mbf = mbf;
    v->has_stereo = true;
    return RSC_OK;
}

// ---- SearchByProjection(pKF, Scw, vpPoints, vpMatched, th) and Fuse(pKF, Scw, vpPoints, th, ...) (rsc_kfproj.h) ----
int rsc_mpview_create(rsc_context* C, const rsc_mappoints* p, rsc_mpview** out) {
    if (!C || !p || !out) return RSC_ERR_ARG;
    *out = nullptr;
    if (p->n < 0) return RSC_ERR_ARG;
    if (p->n > 0 && (!p->state || !p->pos || !p->normal || !p->dmax || !p->dmin || !p->desc)) return RSC_ERR_ARG;
    const size_t n = (size_t)p->n;
    std::unique_ptr<rsc_mpview> v(new rsc_mpview);
    v->ctx = C;
    v->n = v->dev.n = p->n;
    DevKfpPoints& h = v->dev;
    ViewImage img;
    img.put(h.state, p->state, n);
    img.put(h.pos, p->pos, 3 * n);
    img.put(h.normal, p->normal, 3 * n);
    img.put(h.dmax, p->dmax, n);
    img.put(h.dmin, p->dmin, n);
    img.put(h.desc, p->desc, n);
    img.hold<char>(256);  // the spare block every MapPoint view has ended with (n == 0: the whole image)
    if (int e = upload_image(C, v->mem, img)) return e;
    *out = v.release();
    return RSC_OK;
}

void rsc_mpview_destroy(rsc_mpview* v) { destroy_on_stream(v); }

// ---- ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th) (ORBmatcher.cpp:1173-1315, rsc_lastproj.h) ----
int rsc_lastframe_create(rsc_context* C, const rsc_last_frame_slots* s, rsc_lastframe** out) {
    if (!C || !s || !out) return RSC_ERR_ARG;
    *out = nullptr;
    if (s->n < 0) return RSC_ERR_ARG;
    if (s->n > kLastMaxSlots) {
        g_last_error = "LastFrame with more than 8192 slots";
        return RSC_ERR_ARG;
    }
    if (s->n > 0 && (!s->octave || !s->angle || !s->mp_state || !s->mp_pos || !s->mp_desc || !s->mp_has_obs))
        return RSC_ERR_ARG;
    const size_t n = (size_t)s->n;
    std::unique_ptr<rsc_lastframe> v(new rsc_lastframe);
    v->ctx = C;
    v->n = v->dev.n = s->n;
    DevLastFrame& h = v->dev;
    ViewImage img;
    img.put(h.octave, s->octave, n);
    img.put(h.angle, s->angle, n);
    img.put(h.mp_state, s->mp_state, n);
    img.put(h.mp_pos, s->mp_pos, 3 * n);
    img.put(h.mp_desc, s->mp_desc, n);
    img.put(h.mp_has_obs, s->mp_has_obs, n);
    img.hold<char>(256);  // the spare block every LastFrame view has ended with (n == 0: the whole image)
    if (int e = upload_image(C, v->mem, img)) return e;
    if (n) {
        v->octave.assign(s->octave, s->octave + n);
        v->mp_state.assign(s->mp_state, s->mp_state + n);
        v->mp_has_obs.assign(s->mp_has_obs, s->mp_has_obs + n);
        v->mp_pos.assign(s->mp_pos, s->mp_pos + 3 * n);
    }
    *out = v.release();
    return RSC_OK;
}

void rsc_lastframe_destroy(rsc_lastframe* v) { destroy_on_stream(v); }

// ---- LocalMapping::CreateNewMapPoints: SearchForTriangulation and the triangulation (rsc_triang.h) ----
int rsc_kfview_set_triangulation(rsc_kfview* v, const rsc_kf_triangulation* t) {
    if (!v || !t) return RSC_ERR_ARG;
    const size_t n = (size_t)std::max(v->n, 0);
    if (n && (!t->u_right || !t->depth || !t->kp_raw || !t->cos_parallax_stereo)) return RSC_ERR_ARG;
    TriView& K = v->tri;
    ViewImage img(20 * n + 4 * 256);
    img.put(K.kp_raw, t->kp_raw, 2 * n);
    img.put(K.u_right, t->u_right, n);
    img.put(K.depth, t->depth, n);
    img.put(K.cos_stereo, t->cos_parallax_stereo, n);
    // searches already enqueued on the context stream may still read the data of an earlier call.  The pointers
    // of v->tri are bound before the copy: should the copy fail after tri_mem has grown, they refer to unfilled
    // memory while has_triang keeps its value (a failed hipMemcpy leaves the context unusable anyway)
    if (int e = upload_image(v->ctx, v->tri_mem, img, /*wait=*/true)) return e;
    K.kp = reinterpret_cast<const float*>(v->dev.kp);
    K.octave = v->dev.octave;
    K.scale = v->dev.scale;
    std::memcpy(K.Rcw, v->R, sizeof(K.Rcw));
    std::memcpy(K.tcw, v->t, sizeof(K.tcw));
    std::memcpy(K.Rwc, t->Rwc, sizeof(K.Rwc));
    std::memcpy(K.Ow, t->Ow, sizeof(K.Ow));
    K.fx = v->K[0]; K.fy = v->K[1]; K.cx = v->K[2]; K.cy = v->K[3];
    K.invfx = t->invfx; K.invfy = t->invfy; K.mb = t->mb; K.mbf = t->mbf;
    K.scale_factor = t->scale_factor;
    K.n = v->n;
    K.n_levels = v->dev.n_levels;
    v->h_uright.assign(t->u_right, t->u_right + n);
    std::memcpy(v->Kinv, t->Kinv, sizeof(v->Kinv));
    v->has_triang = true;
    return RSC_OK;
}

}  // extern "C"
