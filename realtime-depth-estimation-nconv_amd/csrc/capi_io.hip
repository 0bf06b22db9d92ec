// capi_io.hip — the extern "C" entry points of the device-side I/O families: loss, metrics, frame ingest
// and export, back-projection, normals, LiDAR projection, colourise, sparsify, occlusion, augment,
// sparsification curves, the IP-Basic baseline, the nearest-sample transform, the view warp with its
// photometric loss, and the depth smoothness loss with its edge weights.
// Host code only: each validates its descriptor, fills the family's argument struct (nconv_internal.h)
// and calls its launcher (capi_common.h).
#include "capi_common.h"

using namespace nconv::capi;

extern "C" {

size_t nconv_depth_loss_workspace_bytes(int B, int H, int W) {
    if (B <= 0 || H <= 0 || W <= 0 || (long long)B * H * W > (1LL << 30)) return 0;
    return nconv::loss_workspace_bytes(B, H, W);
}

// The planes of nconv_depth_loss_fwd / _bwd checked and turned into the kernels' arguments.
static const char* loss_args(const float* r, long long rbs, long long rrs, const float* t, long long tbs,
                             long long trs, int B, int H, int W, size_t ws_bytes, const void* ws, nconv::LossArgs& a) {
    if (!r || !t) return "null plane";
    if (B <= 0 || H <= 0 || W <= 0) return "non-positive B/H/W";
    if ((long long)B * H * W > (1LL << 30)) return "batch too large";
    a.B = B, a.H = H, a.W = W;
    if (const char* why = view_args(r, B, H, W, 4, rbs, rrs, kNoStrideLimit, 16, kViewHW, a.r)) return why;
    if (const char* why = view_args(t, B, H, W, 4, tbs, trs, kNoStrideLimit, 16, kViewHW, a.t)) return why;
    if (!ws || ws_bytes < nconv::loss_workspace_bytes(B, H, W)) return "workspace too small";
    return nullptr;
}

int nconv_depth_loss_fwd(const float* r, long long r_image_stride, long long r_row_stride, const float* t,
                         long long t_image_stride, long long t_row_stride, int B, int H, int W, int use_gradient_loss,
                         float* loss, void* workspace, size_t workspace_bytes, void* stream) {
    const char* fn = "nconv_depth_loss_fwd";
    nconv::LossArgs a;
    if (const char* why = loss_args(r, r_image_stride, r_row_stride, t, t_image_stride, t_row_stride, B, H, W,
                                    workspace_bytes, workspace, a))
        return fail(-22, fn, why);
    if (!loss) return fail(-22, fn, "null loss");
    return launched(fn, nconv::launch_loss_fwd, a, use_gradient_loss != 0, loss, (float*)workspace,
                    (hipStream_t)stream);
}

int nconv_depth_loss_bwd(const float* r, long long r_image_stride, long long r_row_stride, const float* t,
                         long long t_image_stride, long long t_row_stride, int B, int H, int W, int use_gradient_loss,
                         const float* gloss, const void* workspace, size_t workspace_bytes, float* g, void* stream) {
    const char* fn = "nconv_depth_loss_bwd";
    nconv::LossArgs a;
    if (const char* why = loss_args(r, r_image_stride, r_row_stride, t, t_image_stride, t_row_stride, B, H, W,
                                    workspace_bytes, workspace, a))
        return fail(-22, fn, why);
    if (!g) return fail(-22, fn, "null g");
    return launched(fn, nconv::launch_loss_bwd, a, use_gradient_loss != 0, gloss, (const float*)workspace, g,
                    (hipStream_t)stream);
}

size_t nconv_conf_loss_workspace_bytes(int B, int H, int W) {
    if (B <= 0 || H <= 0 || W <= 0 || (long long)B * H * W > (1LL << 30)) return 0;
    return nconv::conf_loss_workspace_bytes(B, H, W);
}

// The operands of nconv_conf_loss_fwd / _bwd checked and turned into the kernels' arguments.
static const char* conf_loss_args(const float* r, long long rbs, long long rrs, const float* c, long long cbs,
                                  long long crs, const float* t, long long tbs, long long trs, int B, int H, int W,
                                  int kind, float beta, const float* lam, nconv::ConfLossArgs& a) {
    if (!r || !c || !t) return "null plane";
    if (!lam) return "null lam";
    if (B <= 0 || H <= 0 || W <= 0) return "non-positive B/H/W";
    if ((long long)B * H * W > (1LL << 30)) return "batch too large";
    if (kind != NCONV_CONF_LOSS_SMOOTH_L1 && kind != NCONV_CONF_LOSS_L2) return "unknown err_kind (enum nconv_conf_loss_err)";
    if (!(beta > 0.f)) return "beta must be positive";
    a.B = B, a.H = H, a.W = W, a.kind = kind, a.beta = beta, a.lam = lam;
    if (const char* why = view_args(r, B, H, W, 4, rbs, rrs, kNoStrideLimit, 16, kViewHW, a.r)) return why;
    if (const char* why = view_args(c, B, H, W, 4, cbs, crs, kNoStrideLimit, 16, kViewHW, a.c)) return why;
    if (const char* why = view_args(t, B, H, W, 4, tbs, trs, kNoStrideLimit, 16, kViewHW, a.t)) return why;
    return nullptr;
}

int nconv_conf_loss_fwd(const float* r, long long r_image_stride, long long r_row_stride, const float* c,
                        long long c_image_stride, long long c_row_stride, const float* t, long long t_image_stride,
                        long long t_row_stride, int B, int H, int W, int err_kind, float beta, const float* lam,
                        float* loss, void* workspace, size_t workspace_bytes, void* stream) {
    const char* fn = "nconv_conf_loss_fwd";
    nconv::ConfLossArgs a;
    if (const char* why = conf_loss_args(r, r_image_stride, r_row_stride, c, c_image_stride, c_row_stride, t,
                                         t_image_stride, t_row_stride, B, H, W, err_kind, beta, lam, a))
        return fail(-22, fn, why);
    if (!loss) return fail(-22, fn, "null loss");
    if (!workspace || workspace_bytes < nconv::conf_loss_workspace_bytes(B, H, W))
        return fail(-22, fn, "workspace too small");
    if ((size_t)workspace % 8) return fail(-22, fn, "workspace not 8-byte aligned");
    return launched(fn, nconv::launch_conf_loss_fwd, a, loss, workspace, (hipStream_t)stream);
}

int nconv_conf_loss_bwd(const float* r, long long r_image_stride, long long r_row_stride, const float* c,
                        long long c_image_stride, long long c_row_stride, const float* t, long long t_image_stride,
                        long long t_row_stride, int B, int H, int W, int err_kind, float beta, const float* lam,
                        const float* gloss, float* g_r, float* g_c, void* stream) {
    const char* fn = "nconv_conf_loss_bwd";
    nconv::ConfLossArgs a;
    if (const char* why = conf_loss_args(r, r_image_stride, r_row_stride, c, c_image_stride, c_row_stride, t,
                                         t_image_stride, t_row_stride, B, H, W, err_kind, beta, lam, a))
        return fail(-22, fn, why);
    if (!g_r && !g_c) return fail(-22, fn, "null g_r and g_c");
    return launched(fn, nconv::launch_conf_loss_bwd, a, gloss, g_r, g_c, (hipStream_t)stream);
}

size_t nconv_depth_metrics_workspace_bytes(int B, int H, int W) {
    if (B <= 0 || H <= 0 || W <= 0 || (long long)B * H * W > (1LL << 30)) return 0;
    return nconv::metrics_workspace_bytes(B, H, W);
}

int nconv_depth_metrics(const float* pred, long long p_image_stride, long long p_row_stride, const float* gt,
                        long long g_image_stride, long long g_row_stride, int B, int H, int W, float gt_min,
                        float gt_max, float clamp_lo, float clamp_hi, double* sums, double* accum, void* workspace,
                        size_t workspace_bytes, void* stream) {
    const char* fn = "nconv_depth_metrics";
    if (!pred || !gt) return fail(-22, fn, "null plane");
    if (!sums && !accum) return fail(-22, fn, "null sums and accum");
    if (B <= 0 || H <= 0 || W <= 0) return fail(-22, fn, "non-positive B/H/W");
    if ((long long)B * H * W > (1LL << 30)) return fail(-22, fn, "batch too large");
    nconv::MetricsArgs a;
    a.B = B, a.H = H, a.W = W;
    if (const char* why = view_args(pred, B, H, W, 4, p_image_stride, p_row_stride, 1LL << 31, 16, kViewHW, a.p))
        return fail(-22, fn, why);
    if (const char* why = view_args(gt, B, H, W, 4, g_image_stride, g_row_stride, 1LL << 31, 16, kViewHW, a.g))
        return fail(-22, fn, why);
    if (!(gt_min >= 0.f) || !(gt_max >= 0.f) || !(clamp_lo >= 0.f) || !(clamp_hi >= 0.f))
        return fail(-22, fn, "negative or NaN bound");
    if (gt_min > 0.f && gt_max > 0.f && gt_min > gt_max) return fail(-22, fn, "gt_min > gt_max");
    if (clamp_lo > 0.f && clamp_hi > 0.f && clamp_lo > clamp_hi) return fail(-22, fn, "clamp_lo > clamp_hi");
    if (!workspace || workspace_bytes < nconv::metrics_workspace_bytes(B, H, W))
        return fail(-22, fn, "workspace too small");
    if ((size_t)workspace % 8 || (size_t)sums % 8 || (size_t)accum % 8)
        return fail(-22, fn, "workspace / sums / accum not 8-byte aligned");
    const float inf = __builtin_inff();
    a.g_lo = gt_min, a.g_hi = gt_max > 0.f ? gt_max : inf;
    a.c_lo = clamp_lo > 0.f ? clamp_lo : -inf, a.c_hi = clamp_hi > 0.f ? clamp_hi : inf;
    return launched(fn, nconv::launch_metrics, a, sums, accum, workspace, (hipStream_t)stream);
}

int nconv_frame_ingest(const struct nconv_frame_ingest* d, void* stream) {
    const char* fn = "nconv_frame_ingest";
    if (!d) return fail(-22, fn, "null descriptor");
    if (!d->rgb && !d->plane[0].src && !d->plane[1].src) return fail(-22, fn, "nothing to do: no rgb and no planes");
    if (d->B <= 0 || d->h <= 0 || d->w <= 0) return fail(-22, fn, "non-positive B/h/w");
    if ((long long)d->B * d->h * d->w > (1LL << 30)) return fail(-22, fn, "batch too large");
    const int B = d->B, h = d->h, w = d->w;
    // views in bytes (rows of row_bytes one-byte elements), extents below 2^30 bytes
    auto view = [&](const void* base, long long bs, long long rs, long long row_bytes, long long align,
                    nconv::PlaneView& v) {
        return view_args(base, B, h, row_bytes, 1, bs, rs, 1LL << 30, align, kViewBytes, v);
    };
    nconv::IngestArgs a{};
    a.B = B, a.h = h, a.w = w, a.reverse = d->reverse != 0;
    if (d->rgb) {
        if (const char* why = view(d->rgb, d->rgb_image_stride, d->rgb_row_stride, 3LL * w, 4, a.rgb))
            return fail(-22, fn, why);
        if (!d->rgb_out) return fail(-22, fn, "null rgb_out");
        if ((size_t)d->rgb_out % 4) return fail(-22, fn, "rgb_out not 4-byte aligned");
        a.rgb_out = d->rgb_out;
    }
    for (int k = 0; k < 2; ++k) {
        const nconv_frame_plane& p = d->plane[k];
        if (!p.src) continue;
        if (p.dtype != NCONV_FRAME_U8 && p.dtype != NCONV_FRAME_U16 && p.dtype != NCONV_FRAME_F32)
            return fail(-22, fn, "unknown dtype (enum nconv_frame_dtype)");
        const long long E = p.dtype == NCONV_FRAME_U8 ? 1 : p.dtype == NCONV_FRAME_U16 ? 2 : 4;
        if (p.shift < 0 || p.shift > 15) return fail(-22, fn, "shift outside 0..15");
        if (p.dtype == NCONV_FRAME_F32 && p.shift != 0) return fail(-22, fn, "non-zero shift with F32");
        nconv::IngestPlane& q = a.pl[k];
        const long long A = p.dtype == NCONV_FRAME_F32 ? 16 : 4;
        if (const char* why = view(p.src, p.image_stride, p.row_stride, E * w, A, q.src)) return fail(-22, fn, why);
        if ((size_t)p.src % E || q.src.rs % E || q.src.bs % E)
            return fail(-22, fn, "U16 / F32 plane not aligned to its element size");
        if (!p.out) return fail(-22, fn, "null plane out");
        if ((size_t)p.out % 4) return fail(-22, fn, "plane out not 4-byte aligned");
        q.out = p.out, q.dtype = p.dtype, q.shift = p.shift, q.scale = p.scale;
    }
    return launched(fn, nconv::launch_frame_ingest, a, (hipStream_t)stream);
}

int nconv_depth_export_u16(const float* pred, long long image_stride, long long row_stride, int B, int H, int W,
                           float scale, unsigned short* out, void* stream) {
    const char* fn = "nconv_depth_export_u16";
    if (!pred || !out) return fail(-22, fn, "null pred or out");
    if (B <= 0 || H <= 0 || W <= 0) return fail(-22, fn, "non-positive B/H/W");
    if ((long long)B * H * W > (1LL << 30)) return fail(-22, fn, "batch too large");
    nconv::ExportArgs a;
    a.B = B, a.H = H, a.W = W, a.scale = scale, a.out = out;
    if (const char* why = view_args(pred, B, H, W, 4, image_stride, row_stride, 1LL << 31, 16, kViewHW, a.d))
        return fail(-22, fn, why);
    if (!(scale > 0.f) || scale == __builtin_inff()) return fail(-22, fn, "scale must be positive and finite");
    if ((size_t)pred % 4 || (size_t)out % 2) return fail(-22, fn, "pred not 4-byte or out not 2-byte aligned");
    return launched(fn, nconv::launch_depth_export, a, (hipStream_t)stream);
}

// The descriptor of nconv_backproject_map / _points checked and turned into the kernels' arguments
// (with_color: the colour view is needed); NULL, or the reason it is invalid.
static const char* backproject_args(const nconv_backproject* d, bool with_color, nconv::BackprojectArgs& a) {
    if (!d) return "null descriptor";
    if (!d->depth || !d->k) return "null depth or k";
    if (d->B <= 0 || d->H <= 0 || d->W <= 0) return "non-positive B/H/W";
    const int B = d->B, H = d->H, W = d->W;
    if ((long long)B * H * W >= (1LL << 31)) return "batch too large: B * H * W must be below 2^31";
    if (nconv::backproject_segments(B, H, W) > (1LL << 24)) return "batch too large: more than 2^24 segments";
    if (d->k_image_stride < 0) return "negative k image stride";
    // z_max = 0 beside a z_min >= 0 would select nothing: that pair is the absent upper bound
    const float z_max = d->z_max == 0.f && d->z_min >= 0.f ? __FLT_MAX__ : d->z_max;
    if (!(z_max >= d->z_min)) return "z_max < z_min (or NaN)";
    if (d->conf_min != d->conf_min) return "conf_min is NaN";
    // fp32 planes of W elements (128-bit loads), or interleaved bytes (96-bit loads, 4-byte alignment)
    auto view = [&](const void* base, long long bs, long long rs, bool f32, nconv::PlaneView& v) {
        return f32 ? view_args(base, B, H, W, 4, bs, rs, 1LL << 31, 16, kViewPoints, v)
                   : view_args(base, B, H, 3LL * W, 1, bs, rs, 1LL << 31, 4, kViewPoints, v);
    };
    a = nconv::BackprojectArgs{};
    a.B = B, a.H = H, a.W = W, a.nseg = (int)nconv::backproject_segments(B, H, W);
    if (const char* why = view(d->depth, d->depth_image_stride, d->depth_row_stride, true, a.depth)) return why;
    if ((size_t)d->depth % 4 || (size_t)d->k % 4) return "depth or k not 4-byte aligned";
    if (d->conf) {
        if (const char* why = view(d->conf, d->conf_image_stride, d->conf_row_stride, true, a.conf)) return why;
        if ((size_t)d->conf % 4) return "conf not 4-byte aligned";
    }
    if (d->color_kind != NCONV_COLOR_NONE && d->color_kind != NCONV_COLOR_F32_PLANAR &&
        d->color_kind != NCONV_COLOR_U8_INTERLEAVED)
        return "unknown color kind (enum nconv_color_kind)";
    if ((d->color != nullptr) != (d->color_kind != NCONV_COLOR_NONE)) return "color and color_kind: both or neither";
    if (with_color) {
        if (!d->color) return "rgb output without a color source";
        a.color_kind = d->color_kind, a.reverse = d->reverse != 0;
        const bool planar = d->color_kind == NCONV_COLOR_F32_PLANAR;
        if (const char* why = view(d->color, d->color_image_stride, d->color_row_stride, planar, a.color)) return why;
        if (planar) {
            if (d->color_channel_stride < H * d->color_row_stride) return "channel stride smaller than H * row stride";
            if (B > 1 && d->color_image_stride < 2 * d->color_channel_stride + H * d->color_row_stride)
                return "image stride smaller than H * row stride";
            if ((size_t)d->color % 4) return "color not 4-byte aligned";
            a.ocs = d->color_channel_stride;
            a.color.wide = a.color.wide && a.ocs % 4 == 0;
        }
    }
    a.k = d->k, a.kbs = d->k_image_stride;
    a.z_min = d->z_min, a.z_max = z_max, a.conf_min = d->conf_min;
    return nullptr;
}

int nconv_backproject_map(const nconv_backproject* d, float* xyz, void* stream) {
    const char* fn = "nconv_backproject_map";
    nconv::BackprojectArgs a;
    if (const char* why = backproject_args(d, false, a)) return fail(-22, fn, why);
    if (!xyz) return fail(-22, fn, "null xyz");
    if ((size_t)xyz % 4) return fail(-22, fn, "xyz not 4-byte aligned");
    return launched(fn, nconv::launch_backproject_map, a, xyz, (hipStream_t)stream);
}

size_t nconv_backproject_workspace_bytes(int B, int H, int W) {
    if (B <= 0 || H <= 0 || W <= 0 || (long long)B * H * W >= (1LL << 31)) return 0;
    if (nconv::backproject_segments(B, H, W) > (1LL << 24)) return 0;
    return nconv::backproject_workspace_bytes(B, H, W);
}

int nconv_backproject_points(const nconv_backproject* d, float* xyz, unsigned char* rgb, int* index,
                             long long capacity, int* offsets, void* workspace, size_t workspace_bytes,
                             void* stream) {
    const char* fn = "nconv_backproject_points";
    nconv::BackprojectArgs a;
    if (const char* why = backproject_args(d, rgb != nullptr, a)) return fail(-22, fn, why);
    if (capacity < 0) return fail(-22, fn, "negative capacity");
    if (!xyz && capacity > 0) return fail(-22, fn, "null xyz");
    if (!offsets) return fail(-22, fn, "null offsets");
    if ((size_t)xyz % 4 || (size_t)index % 4 || (size_t)offsets % 4)
        return fail(-22, fn, "xyz / index / offsets not 4-byte aligned");
    if (!workspace || workspace_bytes < nconv::backproject_workspace_bytes(a.B, a.H, a.W))
        return fail(-22, fn, "workspace too small");
    if ((size_t)workspace % 4) return fail(-22, fn, "workspace not 4-byte aligned");
    // every rank is below B * H * W < 2^31
    const int cap = (int)(capacity < 0x7fffffffLL ? capacity : 0x7fffffffLL);
    return launched(fn, nconv::launch_backproject_points, a, xyz, rgb, index, cap, offsets, (int*)workspace,
                    (hipStream_t)stream);
}

// nconv_normals_opts checked and turned into the kernels' arguments (NULL: all zero)
static const char* normals_args(const nconv_normals_opts* o, nconv::NormalsArgs& n) {
    n = nconv::NormalsArgs{};
    if (!o) return nullptr;
    if (!(o->jump_rel >= 0.f) || !(o->jump_abs >= 0.f)) return "jump_rel and jump_abs must be >= 0 (and not NaN)";
    n.jump_rel = o->jump_rel, n.jump_abs = o->jump_abs;
    n.gate = o->jump_rel != 0.f || o->jump_abs != 0.f;
    n.empty = (unsigned)o->empty_rgb[0] | ((unsigned)o->empty_rgb[1] << 8) | ((unsigned)o->empty_rgb[2] << 16);
    return nullptr;
}

int nconv_depth_normals(const nconv_backproject* d, const nconv_normals_opts* o, float* normals,
                        unsigned char* image, void* stream) {
    const char* fn = "nconv_depth_normals";
    nconv::BackprojectArgs a;
    nconv::NormalsArgs n;
    if (const char* why = backproject_args(d, false, a)) return fail(-22, fn, why);
    if (const char* why = normals_args(o, n)) return fail(-22, fn, why);
    if (!normals && !image) return fail(-22, fn, "null normals and image: nothing to write");
    if ((size_t)normals % 4) return fail(-22, fn, "normals not 4-byte aligned");
    return launched(fn, nconv::launch_depth_normals, a, n, normals, image, (hipStream_t)stream);
}

int nconv_depth_normals_points(const nconv_backproject* d, const nconv_normals_opts* o, const int* index,
                               const int* offsets, long long capacity, float* normals, void* stream) {
    const char* fn = "nconv_depth_normals_points";
    nconv::BackprojectArgs a;
    nconv::NormalsArgs n;
    if (const char* why = backproject_args(d, false, a)) return fail(-22, fn, why);
    if (const char* why = normals_args(o, n)) return fail(-22, fn, why);
    if (capacity < 0) return fail(-22, fn, "negative capacity");
    if (capacity > 0 && (!index || !offsets || !normals)) return fail(-22, fn, "null index, offsets or normals");
    if ((size_t)index % 4 || (size_t)offsets % 4 || (size_t)normals % 4)
        return fail(-22, fn, "index / offsets / normals not 4-byte aligned");
    if (capacity == 0) return 0;
    // every row is below B * H * W < 2^31
    const int cap = (int)(capacity < 0x7fffffffLL ? capacity : 0x7fffffffLL);
    return launched(fn, nconv::launch_depth_normals_points, a, n, index, offsets, cap, normals, (hipStream_t)stream);
}

size_t nconv_lidar_project_workspace_bytes(int B, int H, int W, int with_index) {
    if (B <= 0 || H <= 0 || W <= 0 || (long long)B * H * W >= (1LL << 31)) return 0;
    return with_index ? (size_t)8 * B * H * W : 0;
}

int nconv_lidar_project(const struct nconv_lidar_project* d, float* depth, int* index, void* workspace,
                        size_t workspace_bytes, void* stream) {
    const char* fn = "nconv_lidar_project";
    if (!d) return fail(-22, fn, "null descriptor");
    if (d->B <= 0 || d->H <= 0 || d->W <= 0) return fail(-22, fn, "non-positive B/H/W");
    if ((long long)d->B * d->H * d->W >= (1LL << 31))
        return fail(-22, fn, "batch too large: B * H * W must be below 2^31");
    if (d->n_rows < 0 || d->n_rows >= (1LL << 31)) return fail(-22, fn, "n_rows must be in [0, 2^31)");
    if (d->point_stride < 3 || d->point_stride > (1 << 20))
        return fail(-22, fn, "point_stride must be in [3, 2^20]");
    if (!d->points && d->n_rows > 0) return fail(-22, fn, "null points");
    if (!d->offsets || !d->m) return fail(-22, fn, "null offsets or m");
    if (!depth) return fail(-22, fn, "null depth");
    if (d->m_image_stride < 0) return fail(-22, fn, "negative m image stride");
    if (!(d->z_min >= 0.f)) return fail(-22, fn, "z_min must be >= 0 (and not NaN)");
    const float z_max = d->z_max == 0.f ? __FLT_MAX__ : d->z_max;
    if (!(z_max >= d->z_min)) return fail(-22, fn, "z_max < z_min (or NaN)");
    if ((size_t)d->points % 4 || (size_t)d->offsets % 4 || (size_t)d->m % 4 || (size_t)depth % 4 || (size_t)index % 4)
        return fail(-22, fn, "points / offsets / m / depth / index not 4-byte aligned");
    if (index) {
        if (!workspace || workspace_bytes < nconv_lidar_project_workspace_bytes(d->B, d->H, d->W, 1))
            return fail(-22, fn, "workspace too small");
        if ((size_t)workspace % 8) return fail(-22, fn, "workspace not 8-byte aligned");
    }
    nconv::LidarArgs a{};
    a.B = d->B, a.H = d->H, a.W = d->W;
    a.n_rows = (int)d->n_rows, a.stride = d->point_stride;
    a.vec = d->point_stride == 4 && (size_t)d->points % 16 == 0;
    a.points = d->points, a.offsets = d->offsets, a.m = d->m, a.mbs = d->m_image_stride;
    a.z_min = d->z_min, a.z_max = z_max;
    return launched(fn, nconv::launch_lidar_project, a, depth, index, index ? (unsigned long long*)workspace : nullptr,
                    (hipStream_t)stream);
}

size_t nconv_depth_colorize_workspace_bytes(int B) { return B > 0 ? (size_t)8 * B : 0; }

int nconv_depth_colorize(const struct nconv_depth_colorize* d, unsigned char* out, void* workspace,
                         size_t workspace_bytes, void* stream) {
    const char* fn = "nconv_depth_colorize";
    if (!d) return fail(-22, fn, "null descriptor");
    if (!d->depth || !out) return fail(-22, fn, "null depth or out");
    if (d->B <= 0 || d->H <= 0 || d->W <= 0) return fail(-22, fn, "non-positive B/H/W");
    if ((long long)d->B * d->H * d->W >= (1LL << 31))
        return fail(-22, fn, "batch too large: B * H * W must be below 2^31");
    if (d->radius < 0 || d->radius > 4) return fail(-22, fn, "radius must be in [0, 4]");
    if (!d->lut && (d->cmap_id < 0 || d->cmap_id > 4))
        return fail(-22, fn, "cmap_id must be in [0, 4] (or give a lut)");
    if (!d->auto_range && (d->vmin != d->vmin || d->vmax != d->vmax)) return fail(-22, fn, "vmin or vmax is NaN");
    if (d->floor != d->floor) return fail(-22, fn, "floor is NaN");
    if (d->auto_range) {
        if (!workspace || workspace_bytes < nconv_depth_colorize_workspace_bytes(d->B))
            return fail(-22, fn, "workspace too small");
        if ((size_t)workspace % 8) return fail(-22, fn, "workspace not 8-byte aligned");
    }
    if ((size_t)d->depth % 4) return fail(-22, fn, "depth not 4-byte aligned");
    nconv::ColorizeArgs a{};
    a.B = d->B, a.H = d->H, a.W = d->W;
    if (const char* why = view_args(d->depth, a.B, a.H, a.W, 4, d->image_stride, d->row_stride, kNoStrideLimit, 16,
                                    kViewPoints, a.d))
        return fail(-22, fn, why);
    if (d->background) {
        if (const char* why = view_args(d->background, a.B, a.H, 3LL * a.W, 1, d->background_image_stride,
                                        d->background_row_stride, kNoStrideLimit, 4, kViewBytes, a.bg))
            return fail(-22, fn, (std::string("background: ") + why).c_str());
    }
    a.lut = d->lut, a.cmap = d->cmap_id, a.auto_range = d->auto_range != 0;
    a.radius = d->radius, a.bgr = d->bgr != 0;
    a.lo = d->vmin, a.hi = d->vmax, a.floor = d->floor;
    const unsigned e0 = d->empty_rgb[a.bgr ? 2 : 0], e1 = d->empty_rgb[1], e2 = d->empty_rgb[a.bgr ? 0 : 2];
    a.empty = e0 | (e1 << 8) | (e2 << 16);
    a.out = out, a.range = a.auto_range ? (unsigned*)workspace : nullptr;
    return launched(fn, nconv::launch_depth_colorize, a, (hipStream_t)stream);
}

size_t nconv_depth_sparsify_workspace_bytes(int B, int H, int W) {
    if (B <= 0 || H <= 0 || W <= 0 || (long long)B * H * W >= (1LL << 31)) return 0;
    return nconv::sparsify_workspace_bytes(B);
}

int nconv_depth_sparsify(const struct nconv_depth_sparsify* d, float* dst, long long dst_image_stride,
                         long long dst_row_stride, int* kept, void* workspace, size_t workspace_bytes,
                         void* stream) {
    const char* fn = "nconv_depth_sparsify";
    if (!d) return fail(-22, fn, "null descriptor");
    if (!d->src || !dst) return fail(-22, fn, "null src or dst");
    if (!d->state) return fail(-22, fn, "null state");
    if (d->B <= 0 || d->H <= 0 || d->W <= 0) return fail(-22, fn, "non-positive B/H/W");
    const int B = d->B, H = d->H, W = d->W;
    if ((long long)B * H * W >= (1LL << 31)) return fail(-22, fn, "batch too large: B * H * W must be below 2^31");
    if (d->mode < NCONV_SPARSIFY_ALL || d->mode > NCONV_SPARSIFY_FRACTION)
        return fail(-22, fn, "unknown mode (enum nconv_sparsify_mode)");
    if (d->mode == NCONV_SPARSIFY_COUNT_DEV && !d->n_dev) return fail(-22, fn, "COUNT_DEV without n_dev");
    if (d->n < 0) return fail(-22, fn, "negative n");
    if (!(d->keep >= 0.f && d->keep <= 1.f))
        return fail(-22, fn, "keep must be in [0, 1] (and not NaN)");
    std::string text;
    auto view = [&](const char* name, long long bs, long long rs, bool zero_bs) {
        // B == 1: the image stride is not read, and a negative one has always passed here
        return flat_view(name, B, H, W, B == 1 && bs < 0 ? 0 : bs, 0, rs, 1, zero_bs, text);
    };
    if (const char* why = view("src", d->src_image_stride, d->src_row_stride, false)) return fail(-22, fn, why);
    if (const char* why = view("dst", dst_image_stride, dst_row_stride, false)) return fail(-22, fn, why);
    if (d->mask)
        if (const char* why = view("mask", d->mask_image_stride, d->mask_row_stride, true)) return fail(-22, fn, why);
    if ((size_t)d->src % 4 || (size_t)dst % 4 || (size_t)d->state % 4 || (size_t)d->n_dev % 4 || (size_t)kept % 4)
        return fail(-22, fn, "src / dst / state / n_dev / kept not 4-byte aligned");
    if (!workspace || workspace_bytes < nconv::sparsify_workspace_bytes(B)) return fail(-22, fn, "workspace too small");
    if ((size_t)workspace % 8) return fail(-22, fn, "workspace not 8-byte aligned");
    const long long sbs = B > 1 ? d->src_image_stride : 0, dbs = B > 1 ? dst_image_stride : 0;
    const bool same = dst == d->src && dst_row_stride == d->src_row_stride && dbs == sbs;
    if (!same && view_extent(dst, B, H, W, dbs, 0, dst_row_stride, 1, 4, "dst")
                     .overlaps(view_extent(d->src, B, H, W, sbs, 0, d->src_row_stride, 1, 4, "src")))
        return fail(-22, fn, "dst overlaps src without being src (same pointer and strides)");
    nconv::SparsifyArgs a{};
    a.B = B, a.H = H, a.W = W, a.mode = d->mode;
    a.src = d->src, a.sbs = sbs, a.srs = d->src_row_stride;
    a.mask = d->mask, a.mbs = B > 1 ? d->mask_image_stride : 0, a.mrs = d->mask_row_stride;
    a.state = d->state, a.n_dev = d->n_dev, a.n = d->n, a.keep = d->keep;
    a.all_pixels = d->all_pixels != 0, a.floor = d->floor;
    a.key_mask = d->key_mask, a.noise_threshold = d->noise_threshold, a.noise_amp = d->noise_amp;
    a.dst = dst, a.dbs = dbs, a.drs = dst_row_stride, a.kept = kept;
    return launched(fn, nconv::launch_depth_sparsify, a, workspace, (hipStream_t)stream);
}

int nconv_depth_occlusion(const struct nconv_depth_occlusion* d, float* dst, long long dst_image_stride,
                          long long dst_row_stride, unsigned char* removed, int* index, int* counts,
                          void* stream) {
    const char* fn = "nconv_depth_occlusion";
    if (!d) return fail(-22, fn, "null descriptor");
    if (!d->src || !dst) return fail(-22, fn, "null src or dst");
    if (d->B <= 0 || d->H <= 0 || d->W <= 0) return fail(-22, fn, "non-positive B/H/W");
    const int B = d->B, H = d->H, W = d->W;
    if ((long long)B * H * W >= (1LL << 31)) return fail(-22, fn, "batch too large: B * H * W must be below 2^31");
    if (d->rh < 0 || d->rh > 16 || d->rw < 0 || d->rw > 16) return fail(-22, fn, "rh and rw must be in [0, 16]");
    if (!(d->jump_abs >= 0.f) || !(d->jump_rel >= 0.f)) return fail(-22, fn, "jump_abs or jump_rel is negative or NaN");
    if (d->floor != d->floor) return fail(-22, fn, "floor is NaN");
    if (d->min_support < 1) return fail(-22, fn, "min_support must be at least 1");
    if ((size_t)d->src % 4 || (size_t)dst % 4 || (size_t)index % 4 || (size_t)counts % 4)
        return fail(-22, fn, "src / dst / index / counts not 4-byte aligned");
    nconv::OcclusionArgs a{};
    a.B = B, a.H = H, a.W = W;
    if (const char* why = view_args(d->src, B, H, W, 4, d->src_image_stride, d->src_row_stride, kNoStrideLimit, 16,
                                    kViewPoints, a.s))
        return fail(-22, fn, (std::string("src: ") + why).c_str());
    nconv::PlaneView dv{};
    if (const char* why = view_args(dst, B, H, W, 4, dst_image_stride, dst_row_stride, kNoStrideLimit, 16, kViewPoints, dv))
        return fail(-22, fn, (std::string("dst: ") + why).c_str());
    // neighbours are read: the byte extents of the two views must be disjoint
    if (view_extent(dst, B, H, W, dv.bs, 0, dv.rs, 1, 4, "dst")
            .overlaps(view_extent(d->src, B, H, W, a.s.bs, 0, a.s.rs, 1, 4, "src")))
        return fail(-22, fn, "dst overlaps src (no in-place operation: neighbours are read)");
    a.rh = d->rh, a.rw = d->rw, a.min_support = d->min_support;
    a.jump_abs = d->jump_abs, a.jump_rel = d->jump_rel, a.floor = d->floor;
    a.dst = dst, a.dbs = dv.bs, a.drs = dv.rs;
    a.removed = removed, a.index = index, a.counts = counts;
    return launched(fn, nconv::launch_depth_occlusion, a, (hipStream_t)stream);
}

int nconv_frame_augment(const struct nconv_frame_augment* d, void* stream) {
    using namespace nconv;
    const char* fn = "nconv_frame_augment";
    auto bad = [&](const char* why) { return fail(-22, fn, why); };
    auto bad_amp = [](float v) { return !(v >= 0.f && v <= 1.f); };
    if (!d) return bad("null descriptor");
    if (!d->state) return bad("null state");
    bool any = d->rgb || d->mask || d->k;
    for (int i = 0; i < 3; ++i) any = any || d->plane[i].src;
    if (!any) return bad("no source at all (rgb, plane, mask or k)");
    if (!d->rgb != !d->rgb_out) return bad("rgb and rgb_out go together: one of them is null");
    for (int i = 0; i < 3; ++i)
        if (!d->plane[i].src != !d->plane[i].out) return bad("a plane's src and out go together: one of them is null");
    if (!d->mask != !d->mask_out) return bad("mask and mask_out go together: one of them is null");
    if (!d->k != !d->k_out) return bad("k and k_out go together: one of them is null");
    if (d->B <= 0 || d->H <= 0 || d->W <= 0 || d->h <= 0 || d->w <= 0) return bad("non-positive B/H/W/h/w");
    const int B = d->B, H = d->H, W = d->W, h = d->h, w = d->w;
    if (h > H || w > W) return bad("the output size (h, w) exceeds the source size (H, W)");
    if ((long long)B * 3 * H * W >= (1LL << 31)) return bad("batch too large: B * 3 * H * W must be below 2^31");
    for (int m : {d->mode_y, d->mode_x})
        if (m < NCONV_AUGMENT_RANDOM || m > NCONV_AUGMENT_MAX) return bad("unknown mode (enum nconv_augment_crop)");
    if (d->flip_threshold > (1ULL << 32)) return bad("flip_threshold above 2^32");
    if (bad_amp(d->brightness) || bad_amp(d->contrast) || bad_amp(d->color))
        return bad("brightness, contrast and color must be in [0, 1] (and not NaN)");
    if (d->pivot != d->pivot || !(d->rgb_max >= 0.f)) return bad("pivot is NaN, or rgb_max is NaN or negative");

    // the views: strides, and the byte extents of every source and output
    std::string text;
    // sources: state, rgb, three planes, mask, k; outputs: rgb, three planes, mask, k, params, gains
    Extent srcs[7], outs[8];
    int ns = 0, no = 0;
    srcs[ns++] = flat_extent(d->state, 12, "state");
    if ((size_t)d->state % 4) return bad("state not 4-byte aligned");
    if (d->rgb) {
        const long long bs = d->rgb_image_stride, cs = d->rgb_channel_stride, rs = d->rgb_row_stride;
        if (const char* why = flat_view("rgb", B, H, W, bs, cs, rs, 3, false, text)) return bad(why);
        if ((size_t)d->rgb % 4 || (size_t)d->rgb_out % 4) return bad("rgb / rgb_out not 4-byte aligned");
        srcs[ns++] = view_extent(d->rgb, B, H, W, bs, cs, rs, 3, 4, "rgb");
        outs[no++] = flat_extent(d->rgb_out, 12LL * B * h * w, "rgb_out");
    }
    static const char* const plane_names[3] = {"plane[0]", "plane[1]", "plane[2]"};
    for (int i = 0; i < 3; ++i) {
        const nconv_augment_plane& pl = d->plane[i];
        if (!pl.src) continue;
        if (const char* why = flat_view(plane_names[i], B, H, W, pl.image_stride, 0, pl.row_stride, 1, false, text))
            return bad(why);
        if ((size_t)pl.src % 4 || (size_t)pl.out % 4) return bad("a plane's src / out not 4-byte aligned");
        srcs[ns++] = view_extent(pl.src, B, H, W, pl.image_stride, 0, pl.row_stride, 1, 4, plane_names[i]);
        outs[no++] = flat_extent(pl.out, 4LL * B * h * w, plane_names[i]);
    }
    if (d->mask) {
        if (const char* why = flat_view("mask", B, H, W, d->mask_image_stride, 0, d->mask_row_stride, 1, true, text))
            return bad(why);
        srcs[ns++] = view_extent(d->mask, B, H, W, d->mask_image_stride, 0, d->mask_row_stride, 1, 1, "mask");
        outs[no++] = flat_extent(d->mask_out, 1LL * B * h * w, "mask_out");
    }
    if (d->k) {
        if ((size_t)d->k % 4 || (size_t)d->k_out % 4) return bad("k / k_out not 4-byte aligned");
        srcs[ns++] = flat_extent(d->k, 36LL * B, "k");
        outs[no++] = flat_extent(d->k_out, 36LL * B, "k_out");
    }
    if ((size_t)d->params % 4 || (size_t)d->gains % 4) return bad("params / gains not 4-byte aligned");
    if (d->params) outs[no++] = flat_extent(d->params, 16LL * B, "params");
    if (d->gains) outs[no++] = flat_extent(d->gains, 20LL * B, "gains");
    for (int i = 0; i < no; ++i)
        for (int j = 0; j < ns; ++j)
            if (outs[i].overlaps(srcs[j])) {
                text = std::string("output ") + outs[i].name + " overlaps source " + srcs[j].name;
                return bad(text.c_str());
            }

    AugmentArgs a{};
    a.B = B, a.H = H, a.W = W, a.h = h, a.w = w;
    a.mode_y = d->mode_y, a.mode_x = d->mode_x, a.flip_threshold = d->flip_threshold;
    a.brightness = d->brightness, a.contrast = d->contrast, a.color = d->color;
    a.pivot = d->pivot, a.rgb_max = d->rgb_max;
    a.jitter = !(d->brightness == 0.f && d->contrast == 0.f && d->color == 0.f);
    a.state = d->state;
    const long long hw = (long long)h * w;
    if (d->rgb)
        for (int c = 0; c < 3; ++c)
            a.slot[a.nslots++] = AugmentSlot{d->rgb + c * d->rgb_channel_stride, d->rgb_out + c * hw,
                                             B > 1 ? d->rgb_image_stride : 0, d->rgb_row_stride, 3 * hw, kRgb, c};
    for (int i = 0; i < 3; ++i)
        if (d->plane[i].src)
            a.slot[a.nslots++] = AugmentSlot{d->plane[i].src, d->plane[i].out, B > 1 ? d->plane[i].image_stride : 0,
                                             d->plane[i].row_stride, hw, kPlane, 0};
    if (d->mask)
        a.slot[a.nslots++] = AugmentSlot{d->mask, d->mask_out, B > 1 ? d->mask_image_stride : 0, d->mask_row_stride,
                                         hw, kMask, 0};
    a.k = d->k, a.k_out = d->k_out, a.params = d->params, a.gains = d->gains;
    return launched(fn, launch_frame_augment, a, (hipStream_t)stream);
}

size_t nconv_depth_sparsification_workspace_bytes(int B, int H, int W, int steps) {
    if (B <= 0 || H <= 0 || W <= 0 || steps < 1 || steps > NCONV_SPARSIFICATION_MAX_STEPS) return 0;
    if ((long long)H * W >= (1LL << 31) || (long long)B * H * W >= (1LL << 31)) return 0;
    return nconv::sparsification_workspace_bytes(B, H, W);
}

int nconv_depth_sparsification(const struct nconv_depth_sparsification* d, void* workspace, size_t workspace_bytes,
                               void* stream) {
    const char* fn = "nconv_depth_sparsification";
    if (!d) return fail(-22, fn, "null descriptor");
    if (!d->pred || !d->gt || !d->conf) return fail(-22, fn, "null plane (pred, gt or conf)");
    if (!d->curves) return fail(-22, fn, "null curves");
    if (d->B <= 0 || d->H <= 0 || d->W <= 0) return fail(-22, fn, "non-positive B/H/W");
    const int B = d->B, H = d->H, W = d->W;
    if (d->steps < 1 || d->steps > NCONV_SPARSIFICATION_MAX_STEPS) return fail(-22, fn, "steps must be in [1, 1024]");
    if ((long long)H * W >= (1LL << 31))
        return fail(-22, fn, "H * W must be below 2^31 (pixel numbers are int32)");
    if ((long long)B * H * W >= (1LL << 31)) return fail(-22, fn, "batch too large: B * H * W must be below 2^31");
    nconv::SparsificationArgs a{};
    a.B = B, a.H = H, a.W = W;
    auto view = [&](const char* name, const float* base, long long bs, long long rs, nconv::PlaneView& v) -> int {
        if (const char* why = view_args(base, B, H, W, 4, bs, rs, 1LL << 31, 16, kViewHW, v))
            return fail(-22, fn, (std::string(name) + ": " + why).c_str());
        return 0;
    };
    if (int rc = view("pred", d->pred, d->pred_image_stride, d->pred_row_stride, a.p)) return rc;
    if (int rc = view("gt", d->gt, d->gt_image_stride, d->gt_row_stride, a.g)) return rc;
    if (int rc = view("conf", d->conf, d->conf_image_stride, d->conf_row_stride, a.c)) return rc;
    if (!(d->gt_min >= 0.f) || !(d->gt_max >= 0.f) || !(d->clamp_lo >= 0.f) || !(d->clamp_hi >= 0.f))
        return fail(-22, fn, "negative or NaN bound");
    if (d->gt_min > 0.f && d->gt_max > 0.f && d->gt_min > d->gt_max) return fail(-22, fn, "gt_min > gt_max");
    if (d->clamp_lo > 0.f && d->clamp_hi > 0.f && d->clamp_lo > d->clamp_hi)
        return fail(-22, fn, "clamp_lo > clamp_hi");
    if ((size_t)d->pred % 4 || (size_t)d->gt % 4 || (size_t)d->conf % 4 || (size_t)d->order % 4)
        return fail(-22, fn, "pred / gt / conf / order not 4-byte aligned");
    if ((size_t)d->curves % 8) return fail(-22, fn, "curves not 8-byte aligned");
    if (!workspace || workspace_bytes < nconv::sparsification_workspace_bytes(B, H, W))
        return fail(-22, fn, "workspace too small");
    if ((size_t)workspace % 8) return fail(-22, fn, "workspace not 8-byte aligned");
    const float inf = __builtin_inff();
    a.g_lo = d->gt_min, a.g_hi = d->gt_max > 0.f ? d->gt_max : inf;
    a.c_lo = d->clamp_lo > 0.f ? d->clamp_lo : -inf, a.c_hi = d->clamp_hi > 0.f ? d->clamp_hi : inf;
    a.steps = d->steps, a.uncertainty = d->uncertainty != 0;
    a.curves = d->curves, a.order = d->order;
    return launched(fn, nconv::launch_depth_sparsification, a, workspace, (hipStream_t)stream);
}

int nconv_depth_ipbasic(const struct nconv_depth_ipbasic* d, float* dst, long long dst_image_stride,
                        long long dst_row_stride, float* work_plane, int* work_top, void* stream) {
    const char* fn = "nconv_depth_ipbasic";
    if (!d) return fail(-22, fn, "null descriptor");
    if (!d->src || !dst) return fail(-22, fn, "null src or dst");
    if (d->B <= 0 || d->H <= 0 || d->W <= 0) return fail(-22, fn, "non-positive B/H/W");
    const int B = d->B, H = d->H, W = d->W;
    if ((long long)B * H * W >= (1LL << 31)) return fail(-22, fn, "batch too large: B * H * W must be below 2^31");
    if (d->kernel_shape < NCONV_IPBASIC_FULL || d->kernel_shape > NCONV_IPBASIC_DIAMOND)
        return fail(-22, fn, "unknown kernel_shape (enum nconv_ipbasic_kernel)");
    if (d->kernel_size != 3 && d->kernel_size != 5 && d->kernel_size != 7)
        return fail(-22, fn, "kernel_size must be 3, 5 or 7");
    if (d->blur != NCONV_IPBASIC_BLUR_NONE && d->blur != NCONV_IPBASIC_BLUR_GAUSSIAN)
        return fail(-22, fn, "unknown blur (enum nconv_ipbasic_blur)");
    // T = 0.1f: below 2 T no depth is a sample
    if (!(d->max_depth > 2.f * 0.1f) || d->max_depth == __builtin_inff())
        return fail(-22, fn, "max_depth must be finite and above 2 T = 0.2");
    if ((size_t)d->src % 4 || (size_t)dst % 4 || (size_t)work_plane % 4 || (size_t)work_top % 4)
        return fail(-22, fn, "src / dst / work_plane / work_top not 4-byte aligned");
    nconv::IpbasicArgs a{};
    a.B = B, a.H = H, a.W = W;
    if (const char* why = view_args(d->src, B, H, W, 4, d->src_image_stride, d->src_row_stride, kNoStrideLimit, 16,
                                    kViewPoints, a.s))
        return fail(-22, fn, (std::string("src: ") + why).c_str());
    nconv::PlaneView dv{};
    if (const char* why = view_args(dst, B, H, W, 4, dst_image_stride, dst_row_stride, kNoStrideLimit, 16, kViewPoints, dv))
        return fail(-22, fn, (std::string("dst: ") + why).c_str());
    // neighbours are read: the byte extents of the two views must be disjoint
    const Extent se = view_extent(d->src, B, H, W, a.s.bs, 0, a.s.rs, 1, 4, "src");
    const Extent de = view_extent(dst, B, H, W, dv.bs, 0, dv.rs, 1, 4, "dst");
    if (de.overlaps(se)) return fail(-22, fn, "dst overlaps src (no in-place operation: neighbours are read)");
    if (d->extrapolate) {
        if (!work_plane || !work_top) return fail(-22, fn, "extrapolate without work_plane and work_top");
        const Extent we = flat_extent(work_plane, 4LL * B * H * W, "work_plane");
        const Extent te = flat_extent(work_top, 4LL * B * W, "work_top");
        if (we.overlaps(se) || we.overlaps(de) || te.overlaps(se) || te.overlaps(de) || we.overlaps(te))
            return fail(-22, fn, "a workspace overlaps src, dst or the other workspace");
        a.work = work_plane, a.top = work_top;
    }
    a.max_depth = d->max_depth, a.shape = d->kernel_shape, a.r1 = d->kernel_size / 2;
    a.extrapolate = d->extrapolate != 0, a.median = d->median != 0, a.blur = d->blur;
    a.keep_samples = d->keep_samples != 0;
    a.dst = dst, a.dbs = dv.bs, a.drs = dv.rs;
    return launched(fn, nconv::launch_depth_ipbasic, a, (hipStream_t)stream);
}

int nconv_depth_nearest(const struct nconv_depth_nearest* d, float* dst, long long dst_image_stride,
                        long long dst_row_stride, int* index, int* dist2, float* dist, int* work, void* stream) {
    const char* fn = "nconv_depth_nearest";
    if (!d) return fail(-22, fn, "null descriptor");
    if (!d->src || !work) return fail(-22, fn, "null src or work");
    if (!dst && !index && !dist2 && !dist) return fail(-22, fn, "no output at all (dst, index, dist2 or dist)");
    if (d->B <= 0 || d->H <= 0 || d->W <= 0) return fail(-22, fn, "non-positive B/H/W");
    const int B = d->B, H = d->H, W = d->W;
    if ((long long)B * H * W >= (1LL << 31)) return fail(-22, fn, "batch too large: B * H * W must be below 2^31");
    if ((long long)H * H + (long long)W * W >= (1LL << 31))
        return fail(-22, fn, "image too large: H^2 + W^2 must be below 2^31 (squared distances are int32)");
    if (d->floor != d->floor) return fail(-22, fn, "floor is NaN");
    if ((size_t)d->src % 4 || (size_t)dst % 4 || (size_t)index % 4 || (size_t)dist2 % 4 || (size_t)dist % 4 ||
        (size_t)work % 4)
        return fail(-22, fn, "src / dst / index / dist2 / dist / work not 4-byte aligned");
    nconv::NearestArgs a{};
    a.B = B, a.H = H, a.W = W;
    if (const char* why = view_args(d->src, B, H, W, 4, d->src_image_stride, d->src_row_stride, kNoStrideLimit, 16,
                                    kViewPoints, a.s))
        return fail(-22, fn, (std::string("src: ") + why).c_str());
    // src, work and the outputs: the byte extents must be pairwise disjoint (other pixels are read)
    const long long plane = 4LL * B * H * W;
    Extent ext[6];
    int n = 0;
    ext[n++] = view_extent(d->src, B, H, W, a.s.bs, 0, a.s.rs, 1, 4, "src");
    ext[n++] = flat_extent(work, plane, "work");
    if (dst) {
        nconv::PlaneView dv{};
        if (const char* why =
                view_args(dst, B, H, W, 4, dst_image_stride, dst_row_stride, kNoStrideLimit, 16, kViewPoints, dv))
            return fail(-22, fn, (std::string("dst: ") + why).c_str());
        a.dst = dst, a.dbs = dv.bs, a.drs = dv.rs;
        ext[n++] = view_extent(dst, B, H, W, dv.bs, 0, dv.rs, 1, 4, "dst");
    }
    if (index) ext[n++] = flat_extent(index, plane, "index");
    if (dist2) ext[n++] = flat_extent(dist2, plane, "dist2");
    if (dist) ext[n++] = flat_extent(dist, plane, "dist");
    for (int i = 1; i < n; ++i)
        for (int j = 0; j < i; ++j)
            if (ext[i].overlaps(ext[j]))
                return fail(-22, fn, (std::string(ext[i].name) + " overlaps " + ext[j].name).c_str());
    a.floor = d->floor, a.max_dist2 = d->max_dist2;
    a.index = index, a.dist2 = dist2, a.dist = dist, a.work = work;
    return launched(fn, nconv::launch_depth_nearest, a, (hipStream_t)stream);
}

// A view of B images of C planes of H rows of W fp32 (nconv_view_warp's src, the loss's tgt) checked and
// turned into the kernels' PlaneView of one plane plus the channel stride: the strides by flat_view, one
// plane's extent by view_args. NULL, or "<name>: <why>" kept in text.
static const char* warp_image_view(const char* name, const float* base, int B, int C, int H, int W, long long bs,
                                   long long cs, long long rs, nconv::PlaneView& v, long long& vcs,
                                   std::string& text) {
    if (const char* why = flat_view(name, B, H, W, B > 1 ? bs : 0, C > 1 ? cs : 0, rs, C, false, text)) return why;
    if (const char* why = view_args(base, 1, H, W, 4, 0, rs, kNoStrideLimit, 16, kViewPoints, v)) {
        text = std::string(name) + ": " + why;
        return text.c_str();
    }
    v.bs = B > 1 ? bs : 0;
    vcs = C > 1 ? cs : 0;
    return nullptr;
}

}  // extern "C"

// The descriptor of nconv_view_warp_* / nconv_photo_loss_* checked and turned into the kernels' arguments
// (declared in capi_common.h: capi_consistency.hip checks its views by it too).
const char* nconv::capi::warp_args(const nconv_view_warp* d, nconv::WarpArgs& a, std::string& text) {
    if (!d) return "null descriptor";
    if (!d->depth || !d->src || !d->k || !d->m) return "null depth, src, k or m";
    if (d->C != 1 && d->C != 3) return "C must be 1 or 3";
    if (d->B <= 0 || d->H <= 0 || d->W <= 0 || d->Hs <= 0 || d->Ws <= 0) return "non-positive B/H/W/Hs/Ws";
    const int B = d->B, C = d->C, H = d->H, W = d->W, Hs = d->Hs, Ws = d->Ws;
    if (H > (1 << 24) || W > (1 << 24) || Hs > (1 << 24) || Ws > (1 << 24))
        return "H, W, Hs and Ws must be at most 2^24 (pixel coordinates are exact floats)";
    if ((long long)B * C * H * W >= (1LL << 31)) return "batch too large: B * C * H * W must be below 2^31";
    if (d->k_image_stride < 0 || d->m_image_stride < 0) return "negative k or m image stride";
    if (!(d->z_min >= 0.f)) return "z_min must be >= 0 (and not NaN)";
    const float z_max = d->z_max == 0.f ? __FLT_MAX__ : d->z_max;
    if (!(z_max >= d->z_min)) return "z_max < z_min (or NaN)";
    if ((size_t)d->depth % 4 || (size_t)d->src % 4 || (size_t)d->k % 4 || (size_t)d->m % 4)
        return "depth / src / k / m not 4-byte aligned";
    a = nconv::WarpArgs{};
    a.B = B, a.C = C, a.H = H, a.W = W, a.Hs = Hs, a.Ws = Ws;
    if (const char* why = view_args(d->depth, B, H, W, 4, d->depth_image_stride, d->depth_row_stride, kNoStrideLimit, 16,
                                    kViewPoints, a.depth)) {
        text = std::string("depth: ") + why;
        return text.c_str();
    }
    if (d->mask) {
        if (const char* why = view_args(d->mask, B, H, W, 1, d->mask_image_stride, d->mask_row_stride, kNoStrideLimit,
                                        4, kViewPoints, a.mask)) {
            text = std::string("mask: ") + why;
            return text.c_str();
        }
    }
    if (const char* why = warp_image_view("src", d->src, B, C, Hs, Ws, d->src_image_stride, d->src_channel_stride,
                                          d->src_row_stride, a.src, a.scs, text))
        return why;
    a.k = d->k, a.kbs = d->k_image_stride, a.m = d->m, a.mbs = d->m_image_stride;
    a.z_min = d->z_min, a.z_max = z_max;
    return nullptr;
}

// NULL, or how view s differs from view 0 in what the views of one call share (kept in text).
const char* nconv::capi::views_agree(const nconv_view_warp* views, int S, std::string& text) {
    const nconv_view_warp& d = views[0];
    for (int s = 1; s < S; ++s) {
        const nconv_view_warp& e = views[s];
        const char* what = nullptr;
        if (e.B != d.B || e.C != d.C || e.H != d.H || e.W != d.W)
            what = "B, C, H or W";
        else if (e.depth != d.depth || e.depth_row_stride != d.depth_row_stride ||
                 (d.B > 1 && e.depth_image_stride != d.depth_image_stride))
            what = "the depth view";
        else if (e.mask != d.mask ||
                 (d.mask && (e.mask_row_stride != d.mask_row_stride ||
                             (d.B > 1 && e.mask_image_stride != d.mask_image_stride))))
            what = "the mask view";
        else if (e.k != d.k || e.k_image_stride != d.k_image_stride)
            what = "k";
        else if (!(e.z_min == d.z_min && e.z_max == d.z_max))
            what = "z_min or z_max";
        if (what) {
            text = "view " + std::to_string(s) + " differs from view 0 in " + what;
            return text.c_str();
        }
    }
    return nullptr;
}

extern "C" {

int nconv_view_warp_fwd(const struct nconv_view_warp* d, float* warped, unsigned char* valid, void* stream) {
    const char* fn = "nconv_view_warp_fwd";
    nconv::WarpArgs a;
    std::string text;
    if (const char* why = warp_args(d, a, text)) return fail(-22, fn, why);
    if (!warped && !valid) return fail(-22, fn, "null warped and valid: nothing to write");
    if ((size_t)warped % 4) return fail(-22, fn, "warped not 4-byte aligned");
    return launched(fn, nconv::launch_view_warp_fwd, a, warped, valid, (hipStream_t)stream);
}

int nconv_view_warp_bwd(const struct nconv_view_warp* d, const float* g_warped, float* g_depth, void* stream) {
    const char* fn = "nconv_view_warp_bwd";
    nconv::WarpArgs a;
    std::string text;
    if (const char* why = warp_args(d, a, text)) return fail(-22, fn, why);
    if (!g_warped || !g_depth) return fail(-22, fn, "null g_warped or g_depth");
    if ((size_t)g_warped % 4 || (size_t)g_depth % 4) return fail(-22, fn, "g_warped / g_depth not 4-byte aligned");
    return launched(fn, nconv::launch_view_warp_bwd, a, g_warped, g_depth, (hipStream_t)stream);
}

size_t nconv_photo_loss_workspace_bytes(int B, int H, int W) {
    if (B <= 0 || H <= 0 || W <= 0 || (long long)B * H * W >= (1LL << 31)) return 0;
    return nconv::photo_loss_workspace_bytes(B, H, W);
}

// The loss's own operands, after warp_args: the target frame and the workspace.
static const char* photo_args(const nconv_view_warp* d, const float* tgt, long long tbs, long long tcs, long long trs,
                              const void* ws, size_t ws_bytes, nconv::WarpArgs& a, std::string& text) {
    if (const char* why = warp_args(d, a, text)) return why;
    if (!tgt) return "null tgt";
    if ((size_t)tgt % 4) return "tgt not 4-byte aligned";
    if (const char* why = warp_image_view("tgt", tgt, a.B, a.C, a.H, a.W, tbs, tcs, trs, a.tgt, a.tcs, text)) return why;
    if (!ws || ws_bytes < nconv::photo_loss_workspace_bytes(a.B, a.H, a.W)) return "workspace too small";
    if ((size_t)ws % 8) return "workspace not 8-byte aligned";
    return nullptr;
}

int nconv_photo_loss_fwd(const struct nconv_view_warp* d, const float* tgt, long long tgt_image_stride,
                         long long tgt_channel_stride, long long tgt_row_stride, float* loss, void* workspace,
                         size_t workspace_bytes, void* stream) {
    const char* fn = "nconv_photo_loss_fwd";
    nconv::WarpArgs a;
    std::string text;
    if (const char* why = photo_args(d, tgt, tgt_image_stride, tgt_channel_stride, tgt_row_stride, workspace,
                                     workspace_bytes, a, text))
        return fail(-22, fn, why);
    if (!loss) return fail(-22, fn, "null loss");
    if ((size_t)loss % 4) return fail(-22, fn, "loss not 4-byte aligned");
    return launched(fn, nconv::launch_photo_loss_fwd, a, loss, workspace, (hipStream_t)stream);
}

int nconv_photo_loss_bwd(const struct nconv_view_warp* d, const float* tgt, long long tgt_image_stride,
                         long long tgt_channel_stride, long long tgt_row_stride, const float* gloss,
                         const void* workspace, size_t workspace_bytes, float* g_depth, void* stream) {
    const char* fn = "nconv_photo_loss_bwd";
    nconv::WarpArgs a;
    std::string text;
    if (const char* why = photo_args(d, tgt, tgt_image_stride, tgt_channel_stride, tgt_row_stride, workspace,
                                     workspace_bytes, a, text))
        return fail(-22, fn, why);
    if (!g_depth) return fail(-22, fn, "null g_depth");
    if ((size_t)gloss % 4 || (size_t)g_depth % 4) return fail(-22, fn, "gloss / g_depth not 4-byte aligned");
    return launched(fn, nconv::launch_photo_loss_bwd, a, gloss, workspace, g_depth, (hipStream_t)stream);
}

size_t nconv_photo_ssim_workspace_bytes(int B, int H, int W) {
    if (B <= 0 || H <= 0 || W <= 0 || (long long)B * H * W >= (1LL << 31)) return 0;
    return nconv::photo_ssim_workspace_bytes(B, H, W);
}

// The SSIM loss's own operands, after warp_args: the target frame, the mixing weight, the constants and
// the workspace.
static const char* ssim_args(const nconv_view_warp* d, const float* tgt, long long tbs, long long tcs, long long trs,
                             float alpha, float c1, float c2, const void* ws, size_t ws_bytes, nconv::WarpArgs& a,
                             std::string& text) {
    if (const char* why = warp_args(d, a, text)) return why;
    if (!tgt) return "null tgt";
    if ((size_t)tgt % 4) return "tgt not 4-byte aligned";
    if (const char* why = warp_image_view("tgt", tgt, a.B, a.C, a.H, a.W, tbs, tcs, trs, a.tgt, a.tcs, text)) return why;
    if (!(alpha >= 0.f && alpha <= 1.f)) return "alpha must be in [0, 1] (and not NaN)";
    if (!(c1 > 0.f && c1 <= __FLT_MAX__) || !(c2 > 0.f && c2 <= __FLT_MAX__)) return "c1 and c2 must be finite and > 0";
    if (!ws || ws_bytes < nconv::photo_ssim_workspace_bytes(a.B, a.H, a.W)) return "workspace too small";
    if ((size_t)ws % 8) return "workspace not 8-byte aligned";
    return nullptr;
}

int nconv_photo_ssim_loss_fwd(const struct nconv_view_warp* d, const float* tgt, long long tgt_image_stride,
                              long long tgt_channel_stride, long long tgt_row_stride, float alpha, float c1, float c2,
                              float* loss, void* workspace, size_t workspace_bytes, void* stream) {
    const char* fn = "nconv_photo_ssim_loss_fwd";
    nconv::WarpArgs a;
    std::string text;
    if (const char* why = ssim_args(d, tgt, tgt_image_stride, tgt_channel_stride, tgt_row_stride, alpha, c1, c2,
                                    workspace, workspace_bytes, a, text))
        return fail(-22, fn, why);
    if (!loss) return fail(-22, fn, "null loss");
    if ((size_t)loss % 4) return fail(-22, fn, "loss not 4-byte aligned");
    return launched(fn, nconv::launch_photo_ssim_loss_fwd, a, alpha, c1, c2, loss, workspace, (hipStream_t)stream);
}

int nconv_photo_ssim_loss_bwd(const struct nconv_view_warp* d, const float* tgt, long long tgt_image_stride,
                              long long tgt_channel_stride, long long tgt_row_stride, float alpha, float c1, float c2,
                              const float* gloss, const void* workspace, size_t workspace_bytes, float* g_depth,
                              void* stream) {
    const char* fn = "nconv_photo_ssim_loss_bwd";
    nconv::WarpArgs a;
    std::string text;
    if (const char* why = ssim_args(d, tgt, tgt_image_stride, tgt_channel_stride, tgt_row_stride, alpha, c1, c2,
                                    workspace, workspace_bytes, a, text))
        return fail(-22, fn, why);
    if (!g_depth) return fail(-22, fn, "null g_depth");
    if ((size_t)gloss % 4 || (size_t)g_depth % 4) return fail(-22, fn, "gloss / g_depth not 4-byte aligned");
    return launched(fn, nconv::launch_photo_ssim_loss_bwd, a, alpha, c1, c2, gloss, workspace, g_depth,
                    (hipStream_t)stream);
}

size_t nconv_photo_min_workspace_bytes(int B, int H, int W) {
    if (B <= 0 || H <= 0 || W <= 0 || (long long)B * H * W >= (1LL << 31)) return 0;
    return nconv::photo_min_workspace_bytes(B, H, W);
}

// The S descriptors of nconv_photo_min_loss_*: each by ssim_args (its own "view s: " in front of the reason),
// then their agreement in everything but the source and its matrix, then auto-masking's equal sizes.
static const char* min_args(const nconv_view_warp* views, int S, const float* tgt, long long tbs, long long tcs,
                            long long trs, float alpha, float c1, float c2, int automask, const void* ws,
                            size_t ws_bytes, nconv::MinArgs& m, std::string& text) {
    if (S < 1 || S > nconv::kMinSources) return "S must be in 1..4";
    if (!views) return "null descriptor";
    if (automask != 0 && automask != 1) return "automask must be 0 or 1";
    m = nconv::MinArgs{};
    for (int s = 0; s < S; ++s) {
        // the workspace's pointer and alignment here; its size, which is this loss's own, below
        if (const char* why = ssim_args(&views[s], tgt, tbs, tcs, trs, alpha, c1, c2, ws, ~(size_t)0, m.v[s], text)) {
            text = "view " + std::to_string(s) + ": " + why;
            return text.c_str();
        }
    }
    const nconv_view_warp& d = views[0];
    if (const char* why = views_agree(views, S, text)) return why;
    if (automask)
        for (int s = 0; s < S; ++s)
            if (views[s].Hs != d.H || views[s].Ws != d.W) {
                text = "automask needs sources of the target's size: view " + std::to_string(s) + " is not (H, W)";
                return text.c_str();
            }
    if (ws_bytes < nconv::photo_min_workspace_bytes(d.B, d.H, d.W)) return "workspace too small";
    m.S = S, m.automask = automask, m.alpha = alpha, m.c1 = c1, m.c2 = c2;
    return nullptr;
}

int nconv_photo_min_loss_fwd(const struct nconv_view_warp* views, int S, const float* tgt,
                             long long tgt_image_stride, long long tgt_channel_stride, long long tgt_row_stride,
                             float alpha, float c1, float c2, int automask, float* loss, unsigned char* winner,
                             float* error, void* workspace, size_t workspace_bytes, void* stream) {
    const char* fn = "nconv_photo_min_loss_fwd";
    nconv::MinArgs m;
    std::string text;
    if (const char* why = min_args(views, S, tgt, tgt_image_stride, tgt_channel_stride, tgt_row_stride, alpha, c1, c2,
                                   automask, workspace, workspace_bytes, m, text))
        return fail(-22, fn, why);
    if (!loss) return fail(-22, fn, "null loss");
    if ((size_t)loss % 4 || (size_t)error % 4) return fail(-22, fn, "loss / error not 4-byte aligned");
    return launched(fn, nconv::launch_photo_min_loss_fwd, m, loss, winner, error, workspace, (hipStream_t)stream);
}

int nconv_photo_min_loss_bwd(const struct nconv_view_warp* views, int S, const float* tgt,
                             long long tgt_image_stride, long long tgt_channel_stride, long long tgt_row_stride,
                             float alpha, float c1, float c2, int automask, const float* gloss,
                             const void* workspace, size_t workspace_bytes, float* g_depth, void* stream) {
    const char* fn = "nconv_photo_min_loss_bwd";
    nconv::MinArgs m;
    std::string text;
    if (const char* why = min_args(views, S, tgt, tgt_image_stride, tgt_channel_stride, tgt_row_stride, alpha, c1, c2,
                                   automask, workspace, workspace_bytes, m, text))
        return fail(-22, fn, why);
    if (!g_depth) return fail(-22, fn, "null g_depth");
    if ((size_t)gloss % 4 || (size_t)g_depth % 4) return fail(-22, fn, "gloss / g_depth not 4-byte aligned");
    return launched(fn, nconv::launch_photo_min_loss_bwd, m, gloss, workspace, g_depth, (hipStream_t)stream);
}

size_t nconv_pose_workspace_bytes(int B, int H, int W) {
    if (B <= 0 || H <= 0 || W <= 0 || (long long)B * H * W >= (1LL << 31)) return 0;
    return nconv::pose_workspace_bytes(B, H, W);
}

// The descriptor of nconv_pose_* and the workspace checked and turned into the kernels' arguments: the
// fields it shares with nconv_view_warp by warp_args, tgt as the photometric loss's, then its own.
static const char* pose_args(const nconv_pose_align* d, const void* ws, size_t ws_bytes, nconv::PoseArgs& a,
                             std::string& text) {
    if (!d) return "null descriptor";
    nconv_view_warp w{};
    w.B = d->B, w.C = d->C, w.H = d->H, w.W = d->W, w.Hs = d->Hs, w.Ws = d->Ws;
    w.depth = d->depth, w.depth_image_stride = d->depth_image_stride, w.depth_row_stride = d->depth_row_stride;
    w.mask = d->mask, w.mask_image_stride = d->mask_image_stride, w.mask_row_stride = d->mask_row_stride;
    w.src = d->src, w.src_image_stride = d->src_image_stride, w.src_channel_stride = d->src_channel_stride;
    w.src_row_stride = d->src_row_stride;
    w.k = d->k, w.k_image_stride = d->k_image_stride, w.m = d->m, w.m_image_stride = d->m_image_stride;
    w.z_min = d->z_min, w.z_max = d->z_max;
    a = nconv::PoseArgs{};
    if (const char* why = warp_args(&w, a.w, text)) return why;
    if (!d->tgt) return "null tgt";
    if ((size_t)d->tgt % 4) return "tgt not 4-byte aligned";
    if (const char* why = warp_image_view("tgt", d->tgt, a.w.B, a.w.C, a.w.H, a.w.W, d->tgt_image_stride,
                                          d->tgt_channel_stride, d->tgt_row_stride, a.w.tgt, a.w.tcs, text))
        return why;
    if (!d->k_src || !d->pose || !d->status || !d->cost || !d->n_hist) return "null k_src, pose, status, cost or n_hist";
    if ((size_t)d->k_src % 4 || (size_t)d->pose % 4 || (size_t)d->status % 4 || (size_t)d->cost % 4 ||
        (size_t)d->n_hist % 4)
        return "k_src / pose / status / cost / n_hist not 4-byte aligned";
    if (d->k_src_image_stride < 0) return "negative k_src image stride";
    if (a.w.B > 1 && d->m_image_stride < 12) return "m_image_stride below 12: the update writes one m per image";
    if (!(d->huber >= 0.f)) return "huber must be >= 0 (and not NaN)";
    if (!(d->damping >= 0.f)) return "damping must be >= 0 (and not NaN)";
    if (d->min_points < 6) return "min_points must be at least 6";
    if (d->history <= 0) return "history must be positive";
    if (!ws || ws_bytes < nconv::pose_workspace_bytes(a.w.B, a.w.H, a.w.W)) return "workspace too small";
    if ((size_t)ws % 8) return "workspace not 8-byte aligned";
    a.k_src = d->k_src, a.ksbs = d->k_src_image_stride;
    a.pose = d->pose, a.m_out = d->m;
    a.huber = d->huber, a.damping = d->damping, a.min_points = d->min_points;
    a.status = d->status, a.cost = d->cost, a.n = d->n_hist, a.history = d->history;
    return nullptr;
}

int nconv_pose_normal_eq(const struct nconv_pose_align* d, void* workspace, size_t workspace_bytes, void* stream) {
    const char* fn = "nconv_pose_normal_eq";
    nconv::PoseArgs a;
    std::string text;
    if (const char* why = pose_args(d, workspace, workspace_bytes, a, text)) return fail(-22, fn, why);
    return launched(fn, nconv::launch_pose_normal_eq, a, workspace, (hipStream_t)stream);
}

int nconv_pose_update(const struct nconv_pose_align* d, void* workspace, size_t workspace_bytes, int it, int apply,
                      void* stream) {
    const char* fn = "nconv_pose_update";
    nconv::PoseArgs a;
    std::string text;
    if (const char* why = pose_args(d, workspace, workspace_bytes, a, text)) return fail(-22, fn, why);
    if (it < 0 || it >= d->history) return fail(-22, fn, "it outside [0, history)");
    return launched(fn, nconv::launch_pose_update, a, workspace, it, apply, (hipStream_t)stream);
}

size_t nconv_smooth_loss_workspace_bytes(int B, int H, int W) {
    if (B <= 0 || H <= 0 || W <= 0 || (long long)B * H * W >= (1LL << 31)) return 0;
    return nconv::smooth_loss_workspace_bytes(B, H, W);
}

// The descriptor of nconv_smooth_loss_* and the workspace checked and turned into the kernels' arguments.
static const char* smooth_args(const nconv_smooth_loss* d, const void* ws, size_t ws_bytes, nconv::SmoothArgs& a,
                               std::string& text) {
    if (!d) return "null descriptor";
    if (!d->depth) return "null depth";
    if (d->order != 1 && d->order != 2) return "order must be 1 or 2";
    if (d->B <= 0 || d->H <= 0 || d->W <= 0) return "non-positive B/H/W";
    const int B = d->B, H = d->H, W = d->W;
    if ((long long)B * H * W >= (1LL << 31)) return "batch too large: B * H * W must be below 2^31";
    if ((size_t)d->depth % 4 || (size_t)d->weights % 4) return "depth / weights not 4-byte aligned";
    a = nconv::SmoothArgs{};
    a.B = B, a.H = H, a.W = W, a.order = d->order, a.w = d->weights;
    if (const char* why = view_args(d->depth, B, H, W, 4, d->depth_image_stride, d->depth_row_stride, kNoStrideLimit, 16,
                                    kViewPoints, a.depth)) {
        text = std::string("depth: ") + why;
        return text.c_str();
    }
    if (d->mask) {
        if (const char* why = view_args(d->mask, B, H, W, 1, d->mask_image_stride, d->mask_row_stride, kNoStrideLimit,
                                        4, kViewPoints, a.mask)) {
            text = std::string("mask: ") + why;
            return text.c_str();
        }
    }
    if (!ws || ws_bytes < nconv::smooth_loss_workspace_bytes(B, H, W)) return "workspace too small";
    if ((size_t)ws % 8) return "workspace not 8-byte aligned";
    return nullptr;
}

int nconv_smooth_loss_fwd(const struct nconv_smooth_loss* d, float* loss, void* workspace, size_t workspace_bytes,
                          void* stream) {
    const char* fn = "nconv_smooth_loss_fwd";
    nconv::SmoothArgs a;
    std::string text;
    if (const char* why = smooth_args(d, workspace, workspace_bytes, a, text)) return fail(-22, fn, why);
    if (!loss) return fail(-22, fn, "null loss");
    if ((size_t)loss % 4) return fail(-22, fn, "loss not 4-byte aligned");
    return launched(fn, nconv::launch_smooth_loss_fwd, a, loss, workspace, (hipStream_t)stream);
}

int nconv_smooth_loss_bwd(const struct nconv_smooth_loss* d, const float* gloss, const void* workspace,
                          size_t workspace_bytes, float* g_depth, void* stream) {
    const char* fn = "nconv_smooth_loss_bwd";
    nconv::SmoothArgs a;
    std::string text;
    if (const char* why = smooth_args(d, workspace, workspace_bytes, a, text)) return fail(-22, fn, why);
    if (!g_depth) return fail(-22, fn, "null g_depth");
    if ((size_t)gloss % 4 || (size_t)g_depth % 4) return fail(-22, fn, "gloss / g_depth not 4-byte aligned");
    // every pixel of g_depth is written while its neighbours' depths are still being read
    const Extent eg = flat_extent(g_depth, (long long)a.B * a.H * a.W * 4, "g_depth");
    if (eg.overlaps(view_extent(d->depth, a.B, a.H, a.W, a.depth.bs, 0, a.depth.rs, 1, 4, "depth")))
        return fail(-22, fn, "g_depth overlaps depth");
    return launched(fn, nconv::launch_smooth_loss_bwd, a, gloss, workspace, g_depth, (hipStream_t)stream);
}

int nconv_edge_weights(const struct nconv_edge_weights* d, float* weights, void* stream) {
    const char* fn = "nconv_edge_weights";
    if (!d) return fail(-22, fn, "null descriptor");
    if (!d->image || !weights) return fail(-22, fn, "null image or weights");
    if (d->C != 1 && d->C != 3) return fail(-22, fn, "C must be 1 or 3");
    if (d->B <= 0 || d->H <= 0 || d->W <= 0) return fail(-22, fn, "non-positive B/H/W");
    if ((long long)d->B * d->C * d->H * d->W >= (1LL << 31))
        return fail(-22, fn, "batch too large: B * C * H * W must be below 2^31");
    if (!(d->alpha >= 0.f) || d->alpha > __FLT_MAX__) return fail(-22, fn, "alpha must be finite and >= 0");
    if ((size_t)d->image % 4 || (size_t)weights % 4) return fail(-22, fn, "image / weights not 4-byte aligned");
    nconv::EdgeArgs a{};
    std::string text;
    a.B = d->B, a.C = d->C, a.H = d->H, a.W = d->W, a.alpha = d->alpha;
    if (const char* why = warp_image_view("image", d->image, a.B, a.C, a.H, a.W, d->image_stride, d->channel_stride,
                                          d->row_stride, a.img, a.cs, text))
        return fail(-22, fn, why);
    const Extent ew = flat_extent(weights, (long long)a.B * 2 * a.H * a.W * 4, "weights");
    if (ew.overlaps(view_extent(d->image, a.B, a.H, a.W, a.img.bs, a.cs, a.img.rs, a.C, 4, "image")))
        return fail(-22, fn, "weights overlaps image");
    return launched(fn, nconv::launch_edge_weights, a, weights, (hipStream_t)stream);
}

}  // extern "C"
