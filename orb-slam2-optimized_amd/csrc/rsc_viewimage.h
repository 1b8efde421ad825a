// rsc_viewimage.h — the host image of a resident view (rsc_views.cpp) and the two argument checks the views
// share, host only and free of HIP.  A view lives in one device allocation: its pieces are laid out on
// 256-byte boundaries in a host image in the order they are put, and the image goes up with one copy
// (upload_image, rsc_host.h).  A builder names the device-pointer field each piece belongs to, and bind() sets
// those fields once the allocation's address is known.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>
#include <utility>
#include <vector>
#include "../../include/rsc.h"
#include "rsc_arena.h"

#pragma GCC visibility push(hidden)  // no instantiation becomes a symbol of the library
namespace rsc {

template <class T>
struct Piece { size_t off; };  // where a piece of T elements starts in the image

struct ViewImage {
    std::vector<char> h;  // zero wherever nothing was copied
    std::vector<std::pair<void*, size_t>> bound;  // (pointer field, offset of the piece it will point at)
    // `expect`: the image's length where the builder can bound it up front (one allocation, not a growing one)
    explicit ViewImage(size_t expect = 0) {
        h.reserve(expect);
        bound.reserve(12);  // what the largest builder names (rsc_kfview_create); more only grows the vector
    }
    // `count` elements at the next 256-byte boundary, left for the caller to fill
    template <class T>
    Piece<T> hold(size_t count) {
        const size_t off = al256(h.size());
        h.resize(off + sizeof(T) * count);
        return {off};
    }
    // the same, copied from src (nothing to copy when count == 0)
    template <class T>
    Piece<T> put(const void* src, size_t count) {
        const Piece<T> p = hold<T>(count);
        if (count) std::memcpy(h.data() + p.off, src, sizeof(T) * count);
        return p;
    }
    // hold / put, and `field` will point at the piece on the device
    template <class T>
    Piece<T> hold(const T*& field, size_t count) {
        bound.emplace_back(&field, al256(h.size()));
        return hold<T>(count);
    }
    template <class T>
    Piece<T> put(const T*& field, const void* src, size_t count) {
        bound.emplace_back(&field, al256(h.size()));
        return put<T>(src, count);
    }
    // every named field = the piece's address in the allocation at d
    void bind(char* d) const {
        for (const auto& b : bound) {
            const char* p = d + b.second;
            std::memcpy(b.first, &p, sizeof(p));
        }
    }
    // closes the image: whole 256-byte blocks and at least one, so an empty view still owns an allocation
    size_t finish() {
        h.resize(std::max(al256(h.size()), (size_t)256));
        return h.size();
    }
};

// the piece at a base address: the host image's or the device allocation's
template <class T>
inline T* at(char* base, Piece<T> p) { return reinterpret_cast<T*>(base + p.off); }

// mGrid as CSR (Frame::mGrid / KeyFrame::mGrid flattened): offsets from 0 and monotone, every index a keypoint
inline int check_grid_csr(const int32_t* cell_begin, const int32_t* cell_feat, int cells, int n, std::string& err) {
    if (cell_begin[0] != 0) return RSC_ERR_ARG;
    for (int c = 0; c < cells; ++c)
        if (cell_begin[c + 1] < cell_begin[c]) return RSC_ERR_ARG;
    const int nf = cell_begin[cells];
    if (nf > 0 && !cell_feat) return RSC_ERR_ARG;
    for (int e = 0; e < nf; ++e)
        if (cell_feat[e] < 0 || cell_feat[e] >= n) {
            err = "mGrid index out of range";
            return RSC_ERR_ARG;
        }
    return 0;
}

// GetFeaturesInArea converts (u - mnMinX + r) * mfGridElementWidthInv to int, undefined out of int's range:
// the u term is below 64 cells, so the radius term r (th or |th|, the caller's choice) times the top
// level's scale is kept below 2^30 cells (rsc.h).  False for a NaN.
inline bool grid_radius_ok(float r, float top_scale, float gw_inv, float gh_inv) {
    return r * top_scale * std::max(gw_inv, gh_inv) < 1073741824.0f;
}

}  // namespace rsc
#pragma GCC visibility pop
