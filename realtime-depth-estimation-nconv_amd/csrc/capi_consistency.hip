// capi_consistency.hip — the extern "C" entry points of the cross-view depth consistency family: the check
// with fusion (nconv_depth_consistency) and the geometry-consistency loss (nconv_geo_consistency_loss_*).
// Host code only: each validates its descriptors by the view warp's own checks (capi_common.h's warp_args,
// views_agree), fills the family's argument struct (nconv_internal.h) and calls its launcher.
#include "capi_common.h"

using namespace nconv::capi;

// One view of the family: everything nconv_view_warp_* refuses, and C == 1 (the source is a depth plane).
static const char* depth_view_args(const nconv_view_warp* d, nconv::WarpArgs& a, std::string& text) {
    if (const char* why = warp_args(d, a, text)) return why;
    if (d->C != 1) return "C must be 1: src is the source view's depth plane";
    return nullptr;
}

extern "C" {

int nconv_depth_consistency(const struct nconv_view_warp* views, const struct nconv_consistency_source* sources,
                            int S, float px_tol, float rel_tol, int min_views, float* fused, unsigned char* count,
                            unsigned char* views_out, float* reproj, float* reldiff, void* stream) {
    const char* fn = "nconv_depth_consistency";
    if (S < 1 || S > nconv::kMinSources) return fail(-22, fn, "S must be in 1..4");
    if (!views || !sources) return fail(-22, fn, "null descriptor");
    nconv::ConsistencyArgs m{};
    std::string text;
    for (int s = 0; s < S; ++s) {
        const char* why = depth_view_args(&views[s], m.v[s], text);
        const nconv_consistency_source& e = sources[s];
        if (!why && (!e.k_src || !e.m_back)) why = "null k_src or m_back";
        if (!why && (e.k_src_image_stride < 0 || e.m_back_image_stride < 0))
            why = "negative k_src or m_back image stride";
        if (!why && ((size_t)e.k_src % 4 || (size_t)e.m_back % 4)) why = "k_src / m_back not 4-byte aligned";
        if (why) {
            text = "view " + std::to_string(s) + ": " + why;
            return fail(-22, fn, text.c_str());
        }
        m.k_src[s] = e.k_src, m.ksbs[s] = e.k_src_image_stride;
        m.m_back[s] = e.m_back, m.mbbs[s] = e.m_back_image_stride;
    }
    if (const char* why = views_agree(views, S, text)) return fail(-22, fn, why);
    if (!(px_tol >= 0.f) || !(rel_tol >= 0.f)) return fail(-22, fn, "px_tol and rel_tol must be >= 0 (and not NaN)");
    if (min_views < 0 || min_views > S) return fail(-22, fn, "min_views must be in 0..S");
    if (!fused && !count && !views_out && !reproj && !reldiff)
        return fail(-22, fn, "null fused, count, views, reproj and reldiff: nothing to write");
    if ((size_t)fused % 4 || (size_t)reproj % 4 || (size_t)reldiff % 4)
        return fail(-22, fn, "fused / reproj / reldiff not 4-byte aligned");
    if ((long long)views[0].B * S * views[0].H * views[0].W >= (1LL << 31))
        return fail(-22, fn, "batch too large: B * S * H * W must be below 2^31");
    m.S = S, m.min_views = min_views, m.px_tol = px_tol, m.rel_tol = rel_tol;
    return launched(fn, nconv::launch_depth_consistency, m, fused, count, views_out, reproj, reldiff,
                    (hipStream_t)stream);
}

size_t nconv_geo_consistency_workspace_bytes(int B, int H, int W) {
    if (B <= 0 || H <= 0 || W <= 0 || (long long)B * H * W >= (1LL << 31)) return 0;
    return nconv::geo_consistency_workspace_bytes(B, H, W);
}

// The loss's operands: the view and the workspace.
static const char* geo_args(const nconv_view_warp* d, const void* ws, size_t ws_bytes, nconv::WarpArgs& a,
                            std::string& text) {
    if (const char* why = depth_view_args(d, a, text)) return why;
    if (!ws || ws_bytes < nconv::geo_consistency_workspace_bytes(a.B, a.H, a.W)) return "workspace too small";
    if ((size_t)ws % 8) return "workspace not 8-byte aligned";
    return nullptr;
}

int nconv_geo_consistency_loss_fwd(const struct nconv_view_warp* d, float* loss, float* diff, void* workspace,
                                   size_t workspace_bytes, void* stream) {
    const char* fn = "nconv_geo_consistency_loss_fwd";
    nconv::WarpArgs a;
    std::string text;
    if (const char* why = geo_args(d, workspace, workspace_bytes, a, text)) return fail(-22, fn, why);
    if (!loss) return fail(-22, fn, "null loss");
    if ((size_t)loss % 4 || (size_t)diff % 4) return fail(-22, fn, "loss / diff not 4-byte aligned");
    return launched(fn, nconv::launch_geo_consistency_loss_fwd, a, loss, diff, workspace, (hipStream_t)stream);
}

int nconv_geo_consistency_loss_bwd(const struct nconv_view_warp* d, const float* gloss, const void* workspace,
                                   size_t workspace_bytes, float* g_depth, void* stream) {
    const char* fn = "nconv_geo_consistency_loss_bwd";
    nconv::WarpArgs a;
    std::string text;
    if (const char* why = geo_args(d, workspace, workspace_bytes, a, text)) return fail(-22, fn, why);
    if (!g_depth) return fail(-22, fn, "null g_depth");
    if ((size_t)gloss % 4 || (size_t)g_depth % 4) return fail(-22, fn, "gloss / g_depth not 4-byte aligned");
    return launched(fn, nconv::launch_geo_consistency_loss_bwd, a, gloss, workspace, g_depth, (hipStream_t)stream);
}

}  // extern "C"
