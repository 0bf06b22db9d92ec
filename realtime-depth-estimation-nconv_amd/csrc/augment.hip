// augment.hip — the training augmentation of a batch (nconv_frame_augment): one random crop window and
// one horizontal flip per image applied alike to the RGB, up to three fp32 planes and a uint8 mask, the
// intrinsics rewritten to match, photometric jitter on the RGB, and a report of what was drawn.
// include/nconv.h states the rule as the contract; augment_params.h holds the draw as code that a host
// program compiles too. The entry point and its validation are in capi_io.hip.
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
#include "augment_params.h"
#include "nconv_internal.h"
#include "plane_io.h"

namespace nconv {

namespace {

constexpr int kT = 256;          // threads: four waves
constexpr int kGroupsPerLane = 4;  // groups of four pixels a lane takes where the plane is large enough
constexpr unsigned kMaxGridZ = 65535u;

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

}  // namespace

int launch_frame_augment(const AugmentArgs& a, hipStream_t st, const char** why) {
    const long long groups = (long long)a.h * ((a.w + 3) / 4);
    const unsigned gx = (unsigned)((groups + (long long)kT * kGroupsPerLane - 1) / ((long long)kT * kGroupsPerLane));
    const dim3 grid(gx, (unsigned)(a.nslots > 0 ? a.nslots : 1), (unsigned)(a.B < (int)kMaxGridZ ? a.B : (int)kMaxGridZ));
    hipLaunchKernelGGL(frame_augment, grid, dim3(kT), 0, st, a);
    return launch_status(why);
}

}  // namespace nconv
