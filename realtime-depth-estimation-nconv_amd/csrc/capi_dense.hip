// capi_dense.hip — the extern "C" entry points of the RGB-guided model's dense layers: weight packing,
// the convolutions and their weight gradient, training-mode BatchNorm, the ReLU + bias backward, the
// one-channel 3x3 convolution and the bilinear resize. Host code only (capi_common.h).
#include "capi_common.h"

using namespace nconv::capi;

namespace {

const char* validate_wgrad(const nconv_dense_wgrad* g) {
    if (!g) return "null descriptor";
    if (g->B <= 0 || g->C0 <= 0 || g->C1 < 0 || g->H <= 0 || g->W <= 0 || g->Cout <= 0)
        return "non-positive B/C0/H/W/Cout";
    if (!g->x0 || (g->C1 > 0 && !g->x1) || !g->gy || !g->gw) return "null pointer";
    if (g->math != NCONV_DENSE_MATH_FP32 && g->math != NCONV_DENSE_MATH_BF16X9 && g->math != NCONV_DENSE_MATH_BF16X6)
        return "unknown math";
    const int cin = g->C0 + g->C1;
    switch (g->kind) {
        case NCONV_DENSE_3X3:
        case NCONV_DENSE_1X1:
            if (g->stride != 1 && g->stride != 2) return "stride must be 1 or 2";
            if (g->Ho != (g->H - 1) / g->stride + 1 || g->Wo != (g->W - 1) / g->stride + 1)
                return "Ho/Wo inconsistent with kind/stride/H/W";
            if (g->Cout > 96) return "weight gradient supports at most 96 output channels";
            if (g->kind == NCONV_DENSE_1X1 && cin > 64) return "1x1 weight gradient supports at most 64 input channels";
            break;
        case NCONV_DENSE_TRANSPOSED_4X4:
            if (g->stride != 2) return "transposed 4x4 has stride 2";
            if ((g->Ho != 2 * g->H && g->Ho != 2 * g->H - 1) || (g->Wo != 2 * g->W && g->Wo != 2 * g->W - 1))
                return "Ho/Wo inconsistent with kind/stride/H/W";
            if (cin > 96) return "transposed weight gradient supports at most 96 input channels";
            break;
        default:
            return "unknown kind (weight gradients: 3x3, 1x1, transposed 4x4)";
    }
    return nullptr;
}

const char* validate_bn(const nconv_bn_train* p) {
    if (!p) return "null descriptor";
    if (p->B <= 0 || p->C <= 0 || p->H <= 0 || p->W <= 0) return "non-positive B/C/H/W";
    if ((long long)p->H * p->W > (1LL << 30)) return "plane too large";
    if (!p->x || !p->mean || !p->invstd) return "null x / mean / invstd";
    if (!(p->eps > 0.f) || p->momentum < 0.f || p->momentum > 1.f) return "eps must be > 0 and momentum in [0, 1]";
    return nullptr;
}

}  // namespace

extern "C" {

size_t nconv_dense_packed_floats(int kind, int Cin, int Cout) {
    if (kind < NCONV_DENSE_3X3 || kind > NCONV_DENSE_CONV4X4_S2 || Cin <= 0 || Cout <= 0) return 0;
    return nconv::dense_packed_floats(kind, Cin, Cout);
}

int nconv_dense_pack(int kind, int Cin, int Cout, const float* w, const float* scale, float* wpack, void* stream) {
    if (kind < NCONV_DENSE_3X3 || kind > NCONV_DENSE_CONV4X4_S2) return fail(-22, "nconv_dense_pack", "unknown kind");
    if (Cin <= 0 || Cout <= 0) return fail(-22, "nconv_dense_pack", "non-positive Cin/Cout");
    if (!w || !wpack) return fail(-22, "nconv_dense_pack", "null weight pointer");
    return launched("nconv_dense_pack", nconv::launch_dense_pack, kind, Cin, Cout, w, scale, wpack,
                    (hipStream_t)stream);
}

int nconv_dense_conv_fwd(const nconv_dense_conv* c, void* stream) {
    const char* fn = "nconv_dense_conv_fwd";
    if (!c) return fail(-22, fn, "null descriptor");
    if (c->B <= 0 || c->H <= 0 || c->W <= 0 || c->C0 <= 0 || c->C1 < 0) return fail(-22, fn, "non-positive B/H/W/C0");
    if (!c->x0 || (c->C1 > 0 && !c->x1)) return fail(-22, fn, "null input pointer");
    if (c->Cout <= 0) return fail(-22, fn, "non-positive Cout");
    if (!c->wpack || !c->out) return fail(-22, fn, "null weight / output pointer");
    if (c->out_c0 < 0 || c->out_c0 + c->Cout > c->out_C) return fail(-22, fn, "output channel range exceeds out_C");
    if (c->math != NCONV_DENSE_MATH_FP32 && c->math != NCONV_DENSE_MATH_BF16X9 && c->math != NCONV_DENSE_MATH_BF16X6)
        return fail(-22, fn, "unknown math");
    int ho, wo;
    switch (c->kind) {
        case NCONV_DENSE_3X3:
            if (c->stride != 1 && c->stride != 2) return fail(-22, fn, "3x3 stride must be 1 or 2");
            ho = (c->H - 1) / c->stride + 1;
            wo = (c->W - 1) / c->stride + 1;
            break;
        case NCONV_DENSE_1X1:
            if (c->stride != 1 && c->stride != 2) return fail(-22, fn, "1x1 stride must be 1 or 2");
            ho = (c->H - 1) / c->stride + 1;
            wo = (c->W - 1) / c->stride + 1;
            if (c->wshort) return fail(-22, fn, "shortcut only with a 3x3 main convolution");
            break;
        case NCONV_DENSE_TRANSPOSED_4X4:
            if (c->stride != 2) return fail(-22, fn, "transposed 4x4 has stride 2");
            if (c->wshort) return fail(-22, fn, "no shortcut for the transposed convolution");
            // 2H x 2W, or cropped by one row / column (the input gradient of a stride-2 conv of
            // an odd-sized input)
            ho = (c->Ho == 2 * c->H - 1) ? c->Ho : 2 * c->H;
            wo = (c->Wo == 2 * c->W - 1) ? c->Wo : 2 * c->W;
            break;
        case NCONV_DENSE_CONV4X4_S2:
            if (c->stride != 2) return fail(-22, fn, "conv 4x4 has stride 2");
            if (c->wshort) return fail(-22, fn, "shortcut only with a 3x3 main convolution");
            ho = (c->H - 1) / 2 + 1;
            wo = (c->W - 1) / 2 + 1;
            break;
        default:
            return fail(-22, fn, "unknown kind");
    }
    if (ho != c->Ho || wo != c->Wo) return fail(-22, fn, "Ho/Wo inconsistent with kind/stride/H/W");
    return launched(fn, nconv::launch_dense_conv, *c, (hipStream_t)stream);
}

size_t nconv_dense_wgrad_workspace_bytes(const nconv_dense_wgrad* g) {
    if (validate_wgrad(g)) return 0;
    return nconv::dense_wgrad_workspace_bytes(*g);
}

int nconv_dense_conv_wgrad(const nconv_dense_wgrad* g, void* workspace, size_t workspace_bytes, void* stream) {
    const char* fn = "nconv_dense_conv_wgrad";
    if (const char* why = validate_wgrad(g)) return fail(-22, fn, why);
    const size_t need = nconv::dense_wgrad_workspace_bytes(*g);
    if (need && (!workspace || workspace_bytes < need)) return fail(-22, fn, "workspace too small");
    return launched(fn, nconv::launch_dense_wgrad, *g, (float*)workspace, workspace_bytes, (hipStream_t)stream);
}

size_t nconv_bn_workspace_bytes(const nconv_bn_train* p) {
    if (validate_bn(p)) return 0;
    return nconv::bn_workspace_bytes(*p);
}

int nconv_bn_train_fwd(const nconv_bn_train* p, void* workspace, size_t workspace_bytes, void* stream) {
    const char* fn = "nconv_bn_train_fwd";
    if (const char* why = validate_bn(p)) return fail(-22, fn, why);
    if (!p->y) return fail(-22, fn, "null y");
    if (!workspace || workspace_bytes < nconv::bn_workspace_bytes(*p)) return fail(-22, fn, "workspace too small");
    return launched(fn, nconv::launch_bn_train_fwd, *p, (float*)workspace, (hipStream_t)stream);
}

int nconv_bn_train_bwd(const nconv_bn_train* p, const float* gy, float* gx, float* ggamma, float* gbeta,
                       void* workspace, size_t workspace_bytes, void* stream) {
    const char* fn = "nconv_bn_train_bwd";
    if (const char* why = validate_bn(p)) return fail(-22, fn, why);
    if (!gy) return fail(-22, fn, "null gy");
    if (!workspace || workspace_bytes < nconv::bn_workspace_bytes(*p)) return fail(-22, fn, "workspace too small");
    return launched(fn, nconv::launch_bn_train_bwd, *p, gy, gx, ggamma, gbeta, (float*)workspace, (hipStream_t)stream);
}

size_t nconv_relu_bias_bwd_workspace_bytes(int B, int C, int H, int W) {
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0) return 0;
    return nconv::relu_bias_workspace_bytes(B, C, H, W);
}

int nconv_relu_bias_bwd(int B, int C, int H, int W, const float* g, const float* out, float* g_masked,
                        float* gbias, void* workspace, size_t workspace_bytes, void* stream) {
    const char* fn = "nconv_relu_bias_bwd";
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0) return fail(-22, fn, "non-positive B/C/H/W");
    if ((long long)H * W > (1LL << 30)) return fail(-22, fn, "plane too large");
    if (!g) return fail(-22, fn, "null g");
    if (!workspace || workspace_bytes < nconv::relu_bias_workspace_bytes(B, C, H, W))
        return fail(-22, fn, "workspace too small");
    return launched(fn, nconv::launch_relu_bias_bwd, B, C, H, W, g, out, g_masked, gbias, (float*)workspace,
                    (hipStream_t)stream);
}

int nconv_conv3x3_c1(const float* x, int B, int Cin, int H, int W, const float* w, const float* res, float* out,
                     void* stream) {
    const char* fn = "nconv_conv3x3_c1";
    if (!x || !w || !out) return fail(-22, fn, "null pointer");
    if (B <= 0 || Cin <= 0 || H <= 0 || W <= 0) return fail(-22, fn, "non-positive B/Cin/H/W");
    return launched(fn, nconv::launch_conv3x3_c1, x, B, Cin, H, W, w, res, out, (hipStream_t)stream);
}

int nconv_bilinear_ac(const float* x, int B, int C, int H, int W, float* y, int Ho, int Wo, void* stream) {
    const char* fn = "nconv_bilinear_ac";
    if (!x || !y) return fail(-22, fn, "null pointer");
    if (B < 0 || C < 0 || H <= 0 || W <= 0 || Ho <= 0 || Wo <= 0) return fail(-22, fn, "bad geometry");
    if ((long long)H * W >= (1LL << 31) || (long long)B * C * Ho * Wo >= (1LL << 40)) return fail(-22, fn, "too large");
    return launched(fn, nconv::launch_bilinear_ac, x, B, C, H, W, y, Ho, Wo, (hipStream_t)stream);
}

}  // extern "C"
