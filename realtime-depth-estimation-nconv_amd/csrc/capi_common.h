// capi_common.h — what the extern "C" boundary files (nconv_capi.hip, capi_dense.hip, capi_io.hip,
// capi_consistency.hip, capi_voxel.hip) share:
// the error text, the launch helper, and the checks of a caller's strided views. The boundary is host
// code only: it validates, fills the launchers' argument structs (nconv_internal.h) and calls a launcher;
// it starts no kernel and calls no runtime function itself.
#pragma once
#include <stdint.h>
#include <string>
#include "nconv_internal.h"

namespace nconv {
namespace capi {

// Records "<fn>: <why>" as the calling thread's nconv_last_error() text and returns code (nconv_capi.hip).
int fail(int code, const char* fn, const char* why);

// One launcher call, launch(args..., &why): 0, or its error recorded under the entry point's name.
template <typename Launch, typename... Args>
int launched(const char* fn, Launch launch, const Args&... args) {
    const char* why = nullptr;
    const int rc = launch(args..., &why);
    return rc ? fail(rc, fn, why) : 0;
}

// The descriptor of the view-warp family checked and turned into the kernels' arguments, and the agreement of
// the S views of one call in what they share (capi_io.hip): NULL, or the reason (kept in text where composed).
const char* warp_args(const nconv_view_warp* d, WarpArgs& a, std::string& text);
const char* views_agree(const nconv_view_warp* views, int S, std::string& text);

// ---- buffer views: 32-bit offsets inside an image, read through a PlaneView (plane_io.h) ------------
// The three reasons a view can be refused, in one entry point's wording.
struct ViewText {
    const char *row, *large, *image;
};
constexpr ViewText kViewHW{"row stride smaller than W", "plane too large", "image stride smaller than H * row stride"};
constexpr ViewText kViewBytes{"row stride smaller than the row's bytes", "plane too large",
                              "image stride smaller than h * row stride"};
constexpr ViewText kViewPoints{"row stride smaller than W", "plane too large: extent of 2^31 bytes or more",
                               "image stride smaller than H * row stride"};
constexpr long long kNoStrideLimit = 0x7fffffffffffffffLL;

// One view of B planes of H rows of `row` elements of `elem` bytes, strides bs / rs in elements, checked
// and turned into the kernels' PlaneView (plane_io.h): NULL, or the reason it is refused. A view's byte
// offsets inside one image are 32-bit (buffer loads) and kOOB must lie past it, so its extent stays
// below 2^31 bytes; `limit` is the entry point's own, older bound on H * rs * elem (kNoStrideLimit:
// the extent alone). The image offsets are 64-bit. `align`: what base and strides must be multiples of,
// in bytes, for the wide loads.
inline const char* view_args(const void* base, int B, int H, long long row, long long elem, long long bs,
                             long long rs, long long limit, long long align, const ViewText& t, PlaneView& v) {
    if (rs < row) return t.row;
    const long long cap = (1LL << 31) / elem;
    if (rs >= limit / elem / H || row >= cap || (H > 1 && rs > (cap - 1 - row) / (H - 1))) return t.large;
    if (B > 1 && bs < H * rs) return t.image;
    v.base = base, v.bs = B > 1 ? bs : 0, v.rs = rs;
    v.wide = (size_t)base % align == 0 && v.rs % (align / elem) == 0 && v.bs % (align / elem) == 0;
    return nullptr;
}

// ---- flat views: 64-bit offsets, no limit on the extent --------------------------------------------
// A view of B images of C channels of H rows of W elements, strides bs / cs / rs in elements (cs is not
// read where C == 1): NULL, or "<name>: <why it is refused>" kept in text. Channels lie inside an image
// or images inside a channel. zero_bs: an image stride of 0 shares one image among the batch. The
// products are taken in 128 bits: counts are below 2^31 and strides at most 2^40.
inline const char* flat_view(const char* name, int B, int H, int W, long long bs, long long cs, long long rs, int C,
                             bool zero_bs, std::string& text) {
    typedef __int128 wide;
    constexpr long long kStrideCap = 1LL << 40;
    const char* why = nullptr;
    const wide plane = (wide)H * rs;  // one channel's rows
    if (rs < W) why = "row stride smaller than W";
    else if (rs > kStrideCap || bs > kStrideCap || cs > kStrideCap || bs < 0 || cs < 0) why = "stride negative or too large";
    else if (C > 1) {
        const bool chan_inner = cs >= plane && (B == 1 || bs >= (wide)(C - 1) * cs + plane);
        const bool chan_outer = B > 1 && bs >= plane && cs >= (wide)(B - 1) * bs + plane;
        if (!chan_inner && !chan_outer) why = cs < plane ? "channel stride smaller than H * row stride (channels overlap)"
                                                          : "image stride too small (images or channels overlap)";
    } else if (B > 1 && !(zero_bs && bs == 0) && bs < plane) {
        why = "image stride smaller than H * row stride";
    }
    if (!why) return nullptr;
    text = std::string(name) + ": " + why;
    return text.c_str();
}

// [lo, hi) of a tensor in bytes, as integers: no arithmetic on the caller's pointers
struct Extent {
    uintptr_t lo, hi;
    const char* name;
    bool overlaps(const Extent& o) const { return lo < o.hi && o.lo < hi; }
};
inline Extent flat_extent(const void* p, long long bytes, const char* name) {
    return Extent{(uintptr_t)p, (uintptr_t)p + (uintptr_t)bytes, name};
}
// of a view as flat_view takes it (B == 1: the image stride is not read), elements of elem bytes
inline Extent view_extent(const void* p, int B, int H, int W, long long bs, long long cs, long long rs, int C,
                          long long elem, const char* name) {
    const uintptr_t last = (uintptr_t)(B - 1) * (uintptr_t)(B > 1 ? bs : 0) + (uintptr_t)(C - 1) * (uintptr_t)cs +
                           (uintptr_t)(H - 1) * (uintptr_t)rs + (uintptr_t)W;
    return Extent{(uintptr_t)p, (uintptr_t)p + last * (uintptr_t)elem, name};
}

}  // namespace capi
}  // namespace nconv
