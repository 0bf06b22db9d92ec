// augment.hip — the training augmentation of a batch (nconv_frame_augment): one random crop window and
// one horizontal flip per image applied alike to the RGB, up to three fp32 planes and a uint8 mask, the
// intrinsics rewritten to match, photometric jitter on the RGB, and a report of what was drawn.
// include/nconv.h states the rule as the contract; augment_params.h holds the draw as code that a host
// program compiles too. The entry point and its validation live here, beside the kernel.
//
//   frame_augment   one launch for every tensor. grid.z enumerates images (a workgroup loops where B
//     exceeds the grid limit), grid.y the tensor slots (each RGB channel, each plane, the mask) and
//     grid.x groups of four consecutive output pixels of one row: a workgroup never straddles an image
//     or a slot, so (y0, x0, flip, gains) and the slot's pointers are wave-uniform and the two Philox
//     blocks are scalar work. A lane reads its four source pixels as one 16-byte load at the row's
//     4-byte alignment (a full group lies inside the source row because x0 + w <= W), reverses them in
//     registers under a flip, applies the jitter on an RGB slot, and stores 16 bytes where the output
//     address allows (the outputs are contiguous, so that depends on w and the row alone). A row's last
//     group of fewer than four pixels, and the mask's bytes, take element loads. Workgroup (0, 0) of
//     an image writes k_out, params and gains.
// No workspace, no atomics, no waiting between workgroups; every output element has one writer.
#include <string>
#include "augment_params.h"
#include "nconv_internal.h"
#include "plane_io.h"

namespace nconv {

namespace {

constexpr int kT = 256;          // threads: four waves
constexpr int kGroupsPerLane = 4;  // groups of four pixels a lane takes where the plane is large enough
constexpr int kMaxSlots = 7;     // three RGB channels, three planes, the mask
constexpr unsigned kMaxGridZ = 65535u;

enum SlotKind { kPlane = 0, kRgb = 1, kMask = 2 };

struct AugmentSlot {
    const void* src;   // image 0 (of this channel)
    void* dst;
    long long bs, rs;  // source strides: elements (bytes for the mask); bs 0 where B == 1
    long long dbs;     // output image stride in elements
    int kind, chan;
};

struct AugmentArgs {
    int B, H, W, h, w;
    int mode_y, mode_x;
    unsigned long long flip_threshold;
    float brightness, contrast, color, pivot, rgb_max;
    int jitter;
    const unsigned* state;
    int nslots;
    AugmentSlot slot[kMaxSlots];
    const float* k;
    float* k_out;
    int* params;
    float* gains;
};

// four fp32 of a row at 4-byte alignment
typedef float f4u __attribute__((ext_vector_type(4), aligned(4)));

__device__ __forceinline__ void small_outputs(const AugmentArgs& a, int b, const nconv_augment_draw& p) {
#pragma clang fp contract(off)
    if (a.k) {
        const float* k = a.k + 9ll * b;
        float* o = a.k_out + 9ll * b;
        const float cx1 = k[2] - (float)p.x0;
        const float cy1 = k[5] - (float)p.y0;
        o[0] = k[0], o[1] = k[1], o[3] = k[3], o[4] = k[4], o[6] = k[6], o[7] = k[7], o[8] = k[8];
        o[2] = p.flip ? (float)(a.w - 1) - cx1 : cx1;
        o[5] = cy1;
    }
    if (a.params) {
        int* o = a.params + 4ll * b;
        o[0] = p.y0, o[1] = p.x0, o[2] = p.flip, o[3] = 0;
    }
    if (a.gains) {
        float* o = a.gains + 5ll * b;
        o[0] = p.g_b, o[1] = p.g_c, o[2] = p.gain[0], o[3] = p.gain[1], o[4] = p.gain[2];
    }
}

__global__ __launch_bounds__(kT) void frame_augment(AugmentArgs a) {
    const int tid = (int)threadIdx.x, slot = (int)blockIdx.y;
    const unsigned gpr = ((unsigned)a.w + 3u) >> 2;  // groups per output row
    const unsigned groups = (unsigned)a.h * gpr;     // h * w < 2^31
    for (int b = (int)blockIdx.z; b < a.B; b += (int)gridDim.z) {
        nconv_augment_draw p;
        nconv_augment_params(a.state, b, a.H, a.W, a.h, a.w, a.mode_y, a.mode_x, a.flip_threshold, a.brightness,
                             a.contrast, a.color, &p);
        if (blockIdx.x == 0 && slot == 0 && tid == 0) small_outputs(a, b, p);
        if (slot >= a.nslots) continue;
        const AugmentSlot s = a.slot[slot];
        const bool jitter = s.kind == kRgb && a.jitter != 0;
        const float gain = s.chan == 0 ? p.gain[0] : s.chan == 1 ? p.gain[1] : p.gain[2];
        for (unsigned g = blockIdx.x * (unsigned)kT + (unsigned)tid; g < groups; g += gridDim.x * (unsigned)kT) {
            const int row = (int)(g / gpr), j = (int)(g - (unsigned)row * gpr) * 4;
            const int n = min(4, a.w - j);
            // the n source pixels in ascending order start at column c; under a flip out[j + q] = run[n - 1 - q]
            const int c = p.flip ? p.x0 + a.w - j - n : p.x0 + j;
            const long long so = (long long)b * s.bs + (long long)(p.y0 + row) * s.rs + c;
            const long long at = (long long)b * s.dbs + (long long)row * a.w + j;
            if (s.kind == kMask) {
                const unsigned char* sp = (const unsigned char*)s.src + so;
                unsigned char* dp = (unsigned char*)s.dst + at;
                unsigned v = 0u;
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    if (q < n) v |= (unsigned)sp[p.flip ? n - 1 - q : q] << (8 * q);
                if (n == 4 && ((size_t)dp & 3) == 0) {
                    *(unsigned*)dp = v;
                } else {
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        if (q < n) dp[q] = (unsigned char)(v >> (8 * q));
                }
                continue;
            }
            const float* sp = (const float*)s.src + so;
            f4 v;
            if (n == 4) {
                const f4u u = *(const f4u*)sp;
                v = p.flip ? f4{u.w, u.z, u.y, u.x} : f4{u.x, u.y, u.z, u.w};
            } else {
                v.x = sp[p.flip ? n - 1 : 0];
                v.y = n > 1 ? sp[p.flip ? n - 2 : 1] : 0.f;
                v.z = n > 2 ? sp[p.flip ? n - 3 : 2] : 0.f;
                v.w = 0.f;
            }
            if (jitter) {
#pragma unroll
                for (int q = 0; q < 4; ++q) v[q] = nconv_augment_jitter(v[q], p.g_b, gain, p.g_c, a.pivot, a.rgb_max);
            }
            store4_f32((float*)s.dst + at, v, n);
        }
    }
}

// [lo, hi) of a tensor in bytes
struct Extent {
    const char *lo, *hi;
    const char* name;
};

bool bad_amp(float v) { return !(v >= 0.f && v <= 1.f); }

}  // namespace

}  // namespace nconv

extern "C" int nconv_frame_augment(const struct nconv_frame_augment* d, void* stream) {
    using namespace nconv;
    const char* fn = "nconv_frame_augment";
    auto fail = [&](const char* why) { return capi_fail(-22, fn, why); };
    if (!d) return fail("null descriptor");
    if (!d->state) return fail("null state");
    bool any = d->rgb || d->mask || d->k;
    for (int i = 0; i < 3; ++i) any = any || d->plane[i].src;
    if (!any) return fail("no source at all (rgb, plane, mask or k)");
    if (!d->rgb != !d->rgb_out) return fail("rgb and rgb_out go together: one of them is null");
    for (int i = 0; i < 3; ++i)
        if (!d->plane[i].src != !d->plane[i].out) return fail("a plane's src and out go together: one of them is null");
    if (!d->mask != !d->mask_out) return fail("mask and mask_out go together: one of them is null");
    if (!d->k != !d->k_out) return fail("k and k_out go together: one of them is null");
    if (d->B <= 0 || d->H <= 0 || d->W <= 0 || d->h <= 0 || d->w <= 0) return fail("non-positive B/H/W/h/w");
    const int B = d->B, H = d->H, W = d->W, h = d->h, w = d->w;
    if (h > H || w > W) return fail("the output size (h, w) exceeds the source size (H, W)");
    if ((long long)B * 3 * H * W >= (1LL << 31)) return fail("batch too large: B * 3 * H * W must be below 2^31");
    for (int m : {d->mode_y, d->mode_x})
        if (m < NCONV_AUGMENT_RANDOM || m > NCONV_AUGMENT_MAX) return fail("unknown mode (enum nconv_augment_crop)");
    if (d->flip_threshold > (1ULL << 32)) return fail("flip_threshold above 2^32");
    if (bad_amp(d->brightness) || bad_amp(d->contrast) || bad_amp(d->color))
        return fail("brightness, contrast and color must be in [0, 1] (and not NaN)");
    if (d->pivot != d->pivot || !(d->rgb_max >= 0.f)) return fail("pivot is NaN, or rgb_max is NaN or negative");

    // the views: strides, and the byte extents of every source and output
    constexpr long long kStrideCap = 1LL << 40;
    std::string text;
    auto view = [&](const char* name, long long bs, long long cs, long long rs, int C, bool zero_bs) -> const char* {
        const char* why = nullptr;
        const long long plane = (long long)H * rs;  // one channel's rows
        if (rs < W) why = "row stride smaller than W";
        else if (rs > kStrideCap || bs > kStrideCap || cs > kStrideCap || bs < 0 || cs < 0) why = "stride negative or too large";
        else if (C > 1) {
            // channels inside an image, or images inside a channel
            const bool chan_inner = cs >= plane && (B == 1 || bs >= (C - 1) * cs + plane);
            const bool chan_outer = B > 1 && bs >= plane && cs >= (B - 1) * bs + plane;
            if (!chan_inner && !chan_outer) why = cs < plane ? "channel stride smaller than H * row stride (channels overlap)"
                                                              : "image stride too small (images or channels overlap)";
        } else if (B > 1 && !(zero_bs && bs == 0) && bs < plane) {
            why = "image stride smaller than H * row stride";
        }
        if (!why) return nullptr;
        text = std::string(name) + ": " + why;
        return text.c_str();
    };
    Extent srcs[6], outs[8];
    int ns = 0, no = 0;
    auto span = [&](const void* p, long long bs, long long cs, long long rs, int C, long long elem) {
        const long long last = (B - 1) * (B > 1 ? bs : 0) + (C - 1) * cs + (long long)(H - 1) * rs + W;
        return Extent{(const char*)p, (const char*)p + last * elem, nullptr};
    };
    auto flat = [&](const void* p, long long bytes, const char* name) {
        return Extent{(const char*)p, (const char*)p + bytes, name};
    };
    srcs[ns++] = flat(d->state, 12, "state");
    if ((size_t)d->state % 4) return fail("state not 4-byte aligned");
    if (d->rgb) {
        if (const char* why = view("rgb", d->rgb_image_stride, d->rgb_channel_stride, d->rgb_row_stride, 3, false))
            return fail(why);
        if ((size_t)d->rgb % 4 || (size_t)d->rgb_out % 4) return fail("rgb / rgb_out not 4-byte aligned");
        srcs[ns] = span(d->rgb, d->rgb_image_stride, d->rgb_channel_stride, d->rgb_row_stride, 3, 4);
        srcs[ns++].name = "rgb";
        outs[no++] = flat(d->rgb_out, 12LL * B * h * w, "rgb_out");
    }
    static const char* const plane_names[3] = {"plane[0]", "plane[1]", "plane[2]"};
    for (int i = 0; i < 3; ++i) {
        const nconv_augment_plane& pl = d->plane[i];
        if (!pl.src) continue;
        if (const char* why = view(plane_names[i], pl.image_stride, 0, pl.row_stride, 1, false)) return fail(why);
        if ((size_t)pl.src % 4 || (size_t)pl.out % 4) return fail("a plane's src / out not 4-byte aligned");
        srcs[ns] = span(pl.src, pl.image_stride, 0, pl.row_stride, 1, 4);
        srcs[ns++].name = plane_names[i];
        outs[no++] = flat(pl.out, 4LL * B * h * w, plane_names[i]);
    }
    if (d->mask) {
        if (const char* why = view("mask", d->mask_image_stride, 0, d->mask_row_stride, 1, true)) return fail(why);
        srcs[ns] = span(d->mask, d->mask_image_stride, 0, d->mask_row_stride, 1, 1);
        srcs[ns++].name = "mask";
        outs[no++] = flat(d->mask_out, 1LL * B * h * w, "mask_out");
    }
    if (d->k) {
        if ((size_t)d->k % 4 || (size_t)d->k_out % 4) return fail("k / k_out not 4-byte aligned");
        srcs[ns++] = flat(d->k, 36LL * B, "k");
        outs[no++] = flat(d->k_out, 36LL * B, "k_out");
    }
    if ((size_t)d->params % 4 || (size_t)d->gains % 4) return fail("params / gains not 4-byte aligned");
    if (d->params) outs[no++] = flat(d->params, 16LL * B, "params");
    if (d->gains) outs[no++] = flat(d->gains, 20LL * B, "gains");
    for (int i = 0; i < no; ++i)
        for (int j = 0; j < ns; ++j)
            if (outs[i].lo < srcs[j].hi && srcs[j].lo < outs[i].hi) {
                text = std::string("output ") + outs[i].name + " overlaps source " + srcs[j].name;
                return fail(text.c_str());
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

    const long long groups = (long long)h * ((w + 3) / 4);
    const unsigned gx = (unsigned)((groups + (long long)kT * kGroupsPerLane - 1) / ((long long)kT * kGroupsPerLane));
    const dim3 grid(gx, (unsigned)(a.nslots > 0 ? a.nslots : 1), (unsigned)(B < (int)kMaxGridZ ? B : (int)kMaxGridZ));
    hipLaunchKernelGGL(frame_augment, grid, dim3(kT), 0, (hipStream_t)stream, a);
    const char* why = nullptr;
    const int rc = launch_status(&why);
    return rc ? capi_fail(rc, fn, why) : 0;
}
