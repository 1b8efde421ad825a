// rsc_mappoints.cpp — the MapPoint update of the C ABI: rsc_update_map_points_many
// (MapPoint::ComputeDistinctiveDescriptors and MapPoint::UpdateNormalAndDepth over a batch, rsc_mpupdate.h)
// and the read-back of a resident MapPoint view.
#include <cstring>
#include <vector>
#include "rsc_host.h"
#include "rsc_mpupdate.h"

extern "C" {

int rsc_mpview_download(rsc_mpview* v, uint8_t* state, float* pos, float* normal, float* dmax, float* dmin,
                        uint8_t* desc) {
    if (!v) return RSC_ERR_ARG;
    const size_t n = (size_t)v->n;
    RSC_HIP(hipSetDevice(v->ctx->device));
    RSC_HIP(hipStreamSynchronize(v->ctx->stream));  // an update enqueued on the context stream lands first
    if (!n) return RSC_OK;
    const DevKfpPoints& d = v->dev;
    if (state) RSC_HIP(hipMemcpy(state, d.state, n, hipMemcpyDeviceToHost));
    if (pos) RSC_HIP(hipMemcpy(pos, d.pos, 12 * n, hipMemcpyDeviceToHost));
    if (normal) RSC_HIP(hipMemcpy(normal, d.normal, 12 * n, hipMemcpyDeviceToHost));
    if (dmax) RSC_HIP(hipMemcpy(dmax, d.dmax, 4 * n, hipMemcpyDeviceToHost));
    if (dmin) RSC_HIP(hipMemcpy(dmin, d.dmin, 4 * n, hipMemcpyDeviceToHost));
    if (desc) RSC_HIP(hipMemcpy(desc, d.desc, 32 * n, hipMemcpyDeviceToHost));
    return RSC_OK;
}

namespace {
int mpu_refuse(const char* why) {
    g_last_error = why;
    return RSC_ERR_ARG;
}
}  // namespace

int rsc_update_map_points_many(rsc_context* C, rsc_kfview* const* kfs, int n_kfs, const rsc_mappoint_updates* in,
                               int what, const rsc_mappoint_update_out* out, rsc_mpview* dst,
                               const int32_t* dst_index) {
    if (!C || !in || n_kfs < 0 || in->n_points < 0) return RSC_ERR_ARG;
    if (what < 1 || what > 3) return mpu_refuse("what is 1 (descriptor), 2 (normal and depth) or 3");
    const int np = in->n_points;
    if (np == 0) return RSC_OK;
    if (!in->obs_begin || (n_kfs && !kfs)) return RSC_ERR_ARG;
    if ((what & 2) && (!in->pos || !in->ref_kf || !in->ref_idx)) return RSC_ERR_ARG;
    if (dst && (dst->ctx != C || !dst_index)) return mpu_refuse("dst of another context, or without dst_index");
    if (in->obs_begin[0] < 0) return mpu_refuse("obs_begin not ascending");
    for (int p = 0; p < np; ++p)
        if (in->obs_begin[p + 1] < in->obs_begin[p]) return mpu_refuse("obs_begin not ascending");
    const int n_obs = in->obs_begin[np];
    if (n_obs > in->obs_begin[0] && (!in->obs_kf || !in->obs_idx)) return RSC_ERR_ARG;
    // the points to update (:233, :238, :320, :327), by class; the observations of KeyFrames that are not bad
    std::vector<int32_t> order, block, kept_begin((size_t)np + 1, 0), kept_pos;
    for (int p = 0; p < np; ++p) {
        kept_begin[p + 1] = kept_begin[p];
        const int ob = in->obs_begin[p], n = in->obs_begin[p + 1] - ob;
        if ((in->skip && in->skip[p]) || n == 0) continue;
        if (n > kMpuMaxObs) return mpu_refuse("an observation list longer than RSC_MPUPDATE_MAX_OBS (1024)");
        for (int i = 0; i < n; ++i) {
            const int k = in->obs_kf[ob + i], idx = in->obs_idx[ob + i];
            if (k < 0 || k >= n_kfs || !kfs[k] || kfs[k]->ctx != C) return mpu_refuse("obs_kf out of range");
            if (idx < 0 || idx >= kfs[k]->n) return mpu_refuse("obs_idx out of range");
            if ((what & 2) && !kfs[k]->has_triang)  // Ow
                return mpu_refuse("a KeyFrame view without rsc_kfview_set_triangulation");
            if (!(in->kf_bad && in->kf_bad[k])) {
                kept_pos.push_back(i);
                ++kept_begin[p + 1];
            }
        }
        if (what & 2) {
            const int k = in->ref_kf[p], idx = in->ref_idx[p];
            if (k < 0 || k >= n_kfs || !kfs[k] || kfs[k]->ctx != C) return mpu_refuse("ref_kf out of range");
            if (idx < 0 || idx >= kfs[k]->n) return mpu_refuse("ref_idx out of range");
            if (!kfs[k]->has_triang) return mpu_refuse("a KeyFrame view without rsc_kfview_set_triangulation");
            const int oct = kfs[k]->octave[idx];
            if (oct < 0 || oct >= kfs[k]->dev.n_levels) return mpu_refuse("the reference keypoint's octave out of range");
        }
        (n <= kMpuWaveObs ? order : block).push_back(p);
    }
    if (dst) {
        std::vector<uint8_t> taken((size_t)dst->n, 0);
        for (int p = 0; p < np; ++p) {
            const int s = dst_index[p];
            if (s < -1 || s >= dst->n) return mpu_refuse("dst_index out of range");
            if (s >= 0 && taken[s]++) return mpu_refuse("two points with one dst_index");
        }
    }
    const int n_wave = (int)order.size(), n_block = (int)block.size();
    order.insert(order.end(), block.begin(), block.end());
    if (out && out->updated) std::memset(out->updated, 0, (size_t)np);
    if (order.empty()) return RSC_OK;
    // layout: KeyFrame table | pos | obs_begin | obs_kf | obs_idx | kept_begin | kept_pos | ref_kf | ref_idx |
    // dst_index | order  (uploaded)  | desc | best_obs | normal | dmax | dmin  (comes back); no scratch
    const size_t n1 = (size_t)np, no = (size_t)std::max(n_obs, 1), nk = std::max(kept_pos.size(), (size_t)1);
    Arena A;
    const size_t o_kfs = A.take(sizeof(MpuKF) * (size_t)std::max(n_kfs, 1));
    const size_t o_pos = A.take(12 * n1), o_ob = A.take(4 * (n1 + 1)), o_okf = A.take(4 * no), o_oidx = A.take(4 * no);
    const size_t o_kb = A.take(4 * (n1 + 1)), o_kp = A.take(4 * nk), o_rkf = A.take(4 * n1), o_ridx = A.take(4 * n1);
    const size_t o_dst = A.take(4 * n1), o_ord = A.take(4 * order.size());
    A.end_upload();
    A.end_scratch();
    const size_t o_desc = A.take(32 * n1), o_best = A.take(4 * n1), o_nrm = A.take(12 * n1), o_dmax = A.take(4 * n1);
    const size_t o_dmin = A.take(4 * n1);
    A.finish();
    MpuProblem Q{};
    auto fill = [&](char* h, char* d) -> int {
        MpuKF* hk = reinterpret_cast<MpuKF*>(h + o_kfs);
        for (int k = 0; k < n_kfs; ++k) {
            MpuKF e{};
            if (kfs[k] && kfs[k]->ctx == C) {
                e.desc = reinterpret_cast<const ProjDesc*>(kfs[k]->dev.desc);
                e.octave = kfs[k]->dev.octave;
                e.scale = kfs[k]->dev.scale;
                e.n_levels = kfs[k]->dev.n_levels;
                if (kfs[k]->has_triang) std::memcpy(e.Ow, kfs[k]->tri.Ow, sizeof(e.Ow));
            }
            hk[k] = e;
        }
        if (in->pos) std::memcpy(h + o_pos, in->pos, 12 * n1);
        std::memcpy(h + o_ob, in->obs_begin, 4 * (n1 + 1));
        if (n_obs > 0) {
            std::memcpy(h + o_okf, in->obs_kf, 4 * (size_t)n_obs);
            std::memcpy(h + o_oidx, in->obs_idx, 4 * (size_t)n_obs);
        }
        std::memcpy(h + o_kb, kept_begin.data(), 4 * (n1 + 1));
        if (!kept_pos.empty()) std::memcpy(h + o_kp, kept_pos.data(), 4 * kept_pos.size());
        if (what & 2) {
            std::memcpy(h + o_rkf, in->ref_kf, 4 * n1);
            std::memcpy(h + o_ridx, in->ref_idx, 4 * n1);
        }
        if (dst) std::memcpy(h + o_dst, dst_index, 4 * n1);
        std::memcpy(h + o_ord, order.data(), 4 * order.size());
        auto i32 = [&](size_t o) { return reinterpret_cast<const int32_t*>(d + o); };
        Q.kfs = reinterpret_cast<const MpuKF*>(d + o_kfs);
        Q.pos = reinterpret_cast<const float*>(d + o_pos);
        Q.obs_begin = i32(o_ob);
        Q.obs_kf = i32(o_okf);
        Q.obs_idx = i32(o_oidx);
        Q.kept_begin = i32(o_kb);
        Q.kept_pos = i32(o_kp);
        Q.ref_kf = i32(o_rkf);
        Q.ref_idx = i32(o_ridx);
        Q.dst_index = dst ? i32(o_dst) : nullptr;
        Q.order = i32(o_ord);
        Q.desc = reinterpret_cast<ProjDesc*>(d + o_desc);
        Q.best_obs = reinterpret_cast<int32_t*>(d + o_best);
        Q.normal = reinterpret_cast<float*>(d + o_nrm);
        Q.dmax = reinterpret_cast<float*>(d + o_dmax);
        Q.dmin = reinterpret_cast<float*>(d + o_dmin);
        if (dst) {  // the view's own allocation
            Q.dst_desc = const_cast<ProjDesc*>(dst->dev.desc);
            Q.dst_normal = const_cast<float*>(dst->dev.normal);
            Q.dst_dmax = const_cast<float*>(dst->dev.dmax);
            Q.dst_dmin = const_cast<float*>(dst->dev.dmin);
        }
        Q.n_wave = n_wave;
        Q.n_block = n_block;
        Q.what = what;
        return 0;
    };
    auto launch = [&](char*) { return launch_mpupdate(Q, C->stream); };
    if (int e = arena_run(C, C->d_fp, C->h_fp, A, fill, launch)) return e;
    if (!out) return RSC_OK;
    const char* h = C->h_fp.p;
    for (int p : order) {
        uint8_t bits = 0;
        if (what & 1) {
            int32_t b;
            std::memcpy(&b, h + o_best + 4 * (size_t)p, 4);
            if (out->best_obs) out->best_obs[p] = b;
            if (b >= 0) {
                bits |= 1;
                if (out->desc) std::memcpy(out->desc + 32 * (size_t)p, h + o_desc + 32 * (size_t)p, 32);
            }
        }
        if (what & 2) {
            bits |= 2;
            if (out->normal) std::memcpy(out->normal + 3 * (size_t)p, h + o_nrm + 12 * (size_t)p, 12);
            if (out->dmax) std::memcpy(out->dmax + p, h + o_dmax + 4 * (size_t)p, 4);
            if (out->dmin) std::memcpy(out->dmin + p, h + o_dmin + 4 * (size_t)p, 4);
        }
        if (out->updated) out->updated[p] = bits;
    }
    return RSC_OK;
}

}  // extern "C"
