// frame_io.hip — raw sensor frames in, 16-bit depth out, one launch each.
//
//   frame_ingest   uint8 interleaved RGB (B, h, w, 3) -> fp32 planar (B, 3, h, w), exactly float(byte),
//                  optionally with the channels reversed, and up to two single-channel planes
//                  (uint8 / uint16 / fp32, any strides) -> fp32 (B, 1, h, w) = float(v >> shift) * scale
//                  (one fp32 multiply). blockIdx.y selects the job (RGB, plane 0, plane 1).
//   depth_export   fp32 (B, 1, H, W) view -> uint16 (B, 1, H, W): q = d * scale (one rounding),
//                  round to nearest even, clamp to [0, 65535], NaN -> 0.
//
// Both work on tiles of 8 rows x 256 pixels: a wave per pair of rows, four consecutive pixels per
// lane, so a wave's stores of one row are one contiguous span (1 KB of fp32 per channel, 512 B of
// uint16) and its loads of one row likewise (768 B of RGB). The sources are views read as plane_io.h
// describes, RGB and fp32 with its loaders; plane_load4 here follows the same rule for the integer
// planes: a 64-bit load of 4 uint16 / a dword of 4 uint8 where base and strides are 4-byte aligned
// and the four pixels lie inside the row, short by short (byte by byte) otherwise.
// Outputs are 128-bit (ingest) / 64-bit (export) stores where the four pixels' address is aligned,
// else per-element (export: aligned pairs as dwords, single uint16 at the row edges).
// No LDS, no atomics, no host synchronisation, no allocation.
#include "nconv_internal.h"

namespace nconv {

typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

constexpr int kIT = 256;             // threads: four waves
constexpr int kIR = 2;               // rows per wave
constexpr int kIH = kIT / 64 * kIR;  // rows per tile
constexpr int kIW = 64 * 4;          // pixels per tile row (four per lane)

__device__ __forceinline__ unsigned ld_u16(__amdgpu_buffer_rsrc_t r, unsigned off) {
    return __builtin_amdgcn_raw_buffer_load_b16(r, off, 0, 0);
}

// byte k (0..11) of three dwords as a float: v_cvt_f32_ubyte{0..3}
__device__ __forceinline__ float byte_f32(const unsigned (&d)[3], int k) {
    return (float)((d[k >> 2] >> ((k & 3) * 8)) & 0xffu);
}

// rows i0 .. i0 + kIR - 1, pixels j .. j + 3 of image b's RGB
__device__ __forceinline__ void ingest_rgb(const IngestArgs& a, int b, int i0, int j) {
    const __amdgpu_buffer_rsrc_t r = bytes_rsrc(a.rgb.image<unsigned char>(b), view_bytes(a.h, a.rgb.rs, 3LL * a.w, 1));
    const int n = min(4, a.w - j);  // <= 0: the lane is past the row
    unsigned d[kIR][3];
#pragma unroll
    for (int rr = 0; rr < kIR; ++rr) {
        const int i = i0 + rr;
        load4_rgb8(r, a.rgb.wide != 0, i < a.h, n, (unsigned)((long long)i * a.rgb.rs + 3LL * j), d[rr]);
    }
#pragma unroll
    for (int rr = 0; rr < kIR; ++rr) {
        const int i = i0 + rr;
        if (i >= a.h) continue;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const f4 v = {byte_f32(d[rr], c), byte_f32(d[rr], 3 + c), byte_f32(d[rr], 6 + c), byte_f32(d[rr], 9 + c)};
            const int oc = a.reverse ? 2 - c : c;
            store4_f32(a.rgb_out + (((size_t)b * 3 + oc) * a.h + i) * a.w + j, v, n);
        }
    }
}

// four values of a plane row as unsigned integers (U8 / U16) or fp32 bits (F32); off = byte offset of
// pixel j; in_row and n as plane_io.h's loaders take them
template <int DT>
__device__ __forceinline__ u32x4 plane_load4(__amdgpu_buffer_rsrc_t r, bool wide, bool in_row, int n, unsigned off) {
    if (DT == NCONV_FRAME_F32) return __builtin_bit_cast(u32x4, load4_f32(r, wide, in_row, n, off));
    u32x4 v;
    if (wide && (!in_row || n == 4 || n <= 0)) {
        const unsigned o = in_row && n == 4 ? off : kOOB;
        if (DT == NCONV_FRAME_U8) {
            const unsigned w = __builtin_amdgcn_raw_buffer_load_b32(r, o, 0, 0);
            v.x = w & 0xffu, v.y = (w >> 8) & 0xffu, v.z = (w >> 16) & 0xffu, v.w = w >> 24;
        } else {
            const u32x2 w = __builtin_amdgcn_raw_buffer_load_b64(r, o, 0, 0);
            v.x = w.x & 0xffffu, v.y = w.x >> 16, v.z = w.y & 0xffffu, v.w = w.y >> 16;
        }
        return v;
    }
    constexpr unsigned E = DT == NCONV_FRAME_U8 ? 1u : 2u;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const unsigned o = in_row && k < n ? off + E * k : kOOB;
        v[k] = DT == NCONV_FRAME_U8 ? ld_u8(r, o) : ld_u16(r, o);
    }
    return v;
}

template <int DT>
__device__ __forceinline__ void ingest_plane(const IngestArgs& a, const IngestPlane& p, int b, int i0, int j) {
    constexpr int E = DT == NCONV_FRAME_U8 ? 1 : DT == NCONV_FRAME_U16 ? 2 : 4;
    const __amdgpu_buffer_rsrc_t r =
        bytes_rsrc(p.src.image<unsigned char>(b), view_bytes(a.h, p.src.rs, (long long)E * a.w, 1));
    const int n = min(4, a.w - j);
    u32x4 v[kIR];
#pragma unroll
    for (int rr = 0; rr < kIR; ++rr) {
        const int i = i0 + rr;
        const unsigned off = (unsigned)((long long)i * p.src.rs + (long long)E * j);
        v[rr] = plane_load4<DT>(r, p.src.wide != 0, i < a.h, n, off);
    }
#pragma unroll
    for (int rr = 0; rr < kIR; ++rr) {
        const int i = i0 + rr;
        if (i >= a.h) continue;
        f4 f;
        if (DT == NCONV_FRAME_F32) {
            f = __builtin_bit_cast(f4, v[rr]) * p.scale;
        } else {
            const u32x4 s = v[rr] >> (unsigned)p.shift;
            f = f4{(float)s.x, (float)s.y, (float)s.z, (float)s.w} * p.scale;
        }
        store4_f32(p.out + ((size_t)b * a.h + i) * a.w + j, f, n);
    }
}

// grid (B * tiles per image, jobs); job0..2: 0 = RGB, 1 / 2 = plane 0 / 1 (the host lists the present ones)
__global__ __launch_bounds__(kIT) void frame_ingest(IngestArgs a, int job0, int job1, int job2) {
    const TileOrigin o = tile_origin<kIH, kIW>(a.h, a.w);
    const int b = o.b, i0 = o.i0 + (threadIdx.x >> 6) * kIR, j = o.j0 + (threadIdx.x & 63) * 4;
    const int job = blockIdx.y == 0 ? job0 : blockIdx.y == 1 ? job1 : job2;
    if (job == 0) {
        ingest_rgb(a, b, i0, j);
        return;
    }
    const IngestPlane& p = job == 1 ? a.pl[0] : a.pl[1];
    if (p.dtype == NCONV_FRAME_U16)
        ingest_plane<NCONV_FRAME_U16>(a, p, b, i0, j);
    else if (p.dtype == NCONV_FRAME_U8)
        ingest_plane<NCONV_FRAME_U8>(a, p, b, i0, j);
    else
        ingest_plane<NCONV_FRAME_F32>(a, p, b, i0, j);
}

// round(d * scale) to nearest even, clamped into [0, 65535]; comparisons, so a NaN becomes 0
__device__ __forceinline__ unsigned export_q(float d, float scale) {
    float q = rintf(d * scale);
    q = q > 0.f ? q : 0.f;
    q = q < 65535.f ? q : 65535.f;
    return (unsigned)q;
}

// pixels k, k + 1 at the 4-byte aligned p: a dword if both are inside the row, else the first alone
__device__ __forceinline__ void export_pair(unsigned short* p, unsigned lo, unsigned hi, int k, int n) {
    if (k + 1 < n)
        *(unsigned*)p = lo | (hi << 16);
    else if (k < n)
        *p = (unsigned short)lo;
}

__global__ __launch_bounds__(kIT) void depth_export(ExportArgs a) {
    const TileOrigin o = tile_origin<kIH, kIW>(a.H, a.W);
    const int b = o.b, i0 = o.i0 + (threadIdx.x >> 6) * kIR, j = o.j0 + (threadIdx.x & 63) * 4;
    const __amdgpu_buffer_rsrc_t r = plane_rsrc(a.d.image<float>(b), view_bytes(a.H, a.d.rs, a.W, 4));
    const int n = min(4, a.W - j);
    f4 v[kIR];
#pragma unroll
    for (int rr = 0; rr < kIR; ++rr) {
        const int i = i0 + rr;
        v[rr] = load4_f32(r, a.d.wide != 0, i < a.H, n, (unsigned)((long long)i * a.d.rs + j) * 4u);
    }
#pragma unroll
    for (int rr = 0; rr < kIR; ++rr) {
        const int i = i0 + rr;
        if (i >= a.H || n <= 0) continue;
        const unsigned q0 = export_q(v[rr].x, a.scale), q1 = export_q(v[rr].y, a.scale);
        const unsigned q2 = export_q(v[rr].z, a.scale), q3 = export_q(v[rr].w, a.scale);
        unsigned short* p = a.out + ((size_t)b * a.H + i) * a.W + j;
        if (n == 4 && ((size_t)p & 7) == 0) {
            *(u32x2*)p = u32x2{q0 | (q1 << 16), q2 | (q3 << 16)};
        } else if (((size_t)p & 2) == 0) {
            export_pair(p, q0, q1, 0, n);
            export_pair(p + 2, q2, q3, 2, n);
        } else {  // the row starts on an odd pixel of its dword: one uint16, then aligned pairs
            *p = (unsigned short)q0;
            export_pair(p + 1, q1, q2, 1, n);
            if (n > 3) p[3] = (unsigned short)q3;
        }
    }
}

int launch_frame_ingest(const IngestArgs& a, hipStream_t st, const char** why) {
    int jobs[3] = {0, 0, 0}, nj = 0;
    if (a.rgb.base) jobs[nj++] = 0;
    if (a.pl[0].src.base) jobs[nj++] = 1;
    if (a.pl[1].src.base) jobs[nj++] = 2;
    hipLaunchKernelGGL(frame_ingest, dim3(a.B * tiles_per_image<kIH, kIW>(a.h, a.w), nj), dim3(kIT), 0, st, a, jobs[0],
                       jobs[1], jobs[2]);
    return launch_status(why);
}

int launch_depth_export(const ExportArgs& a, hipStream_t st, const char** why) {
    hipLaunchKernelGGL(depth_export, dim3(a.B * tiles_per_image<kIH, kIW>(a.H, a.W)), dim3(kIT), 0, st, a);
    return launch_status(why);
}

}  // namespace nconv
