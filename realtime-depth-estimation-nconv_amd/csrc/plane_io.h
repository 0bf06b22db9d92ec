// plane_io.h — reading a strided view of 2-D planes on the device, and the grid of pixel tiles the
// kernels over such planes are launched on, defined once. Every kernel that takes a PlaneView reads it
// through these loaders (the loss, confidence-loss and metrics kernels, frame_io, backproject, normals,
// colorize, occlusion, ipbasic, nearest, augment, view_warp, smooth_loss); the NConv staging (nconv_common.h) and
// lidar_project.hip take the resource constants and ld_f32.
//
// A view is a batch of planes given as (base, image stride, row stride): PlaneView below, checked and
// filled on the host by view_args in capi_common.h. A kernel reads image b through a buffer resource
// over exactly that image's extent,
//   [base + b * image stride, + ((H - 1) * row stride + row elements) * element bytes),
// which the host keeps below 2^31 bytes, so that the byte offset kOOB lies past every resource and a
// load aimed at it returns 0 without touching memory. A lane takes four consecutive pixels of one
// row; in_row says whether that row is inside the plane, n how many of the four are inside the row
// (<= 0: none). Kept apart because n is often shared by the rows a lane reads:
//   wide    one load of all four (128 bits of fp32, 96 bits of interleaved RGB), where the view's
//           `wide` flag says that base and strides keep every such group aligned, and either all four
//           pixels are in the plane (in_row, n == 4) or none is (the load is aimed at kOOB)
//   else    one load per element, each at its own offset or at kOOB
// Either way no load touches a byte outside the extent, and a wide load is issued only when all its
// bytes lie in one row or it is aimed at kOOB; pixels outside the plane read 0.
#pragma once
#include <hip/hip_runtime.h>

typedef float f4 __attribute__((ext_vector_type(4)));

// a byte offset past every resource (their extents are below 2^31 bytes): the load returns 0
constexpr unsigned kOOB = 0x80000000u;

// extent in bytes of H rows of row_elems elements, row_stride elements apart
__host__ __device__ __forceinline__ int view_bytes(int H, long long row_stride, long long row_elems, int elem_bytes) {
    return (int)(((long long)(H - 1) * row_stride + row_elems) * elem_bytes);
}

// raw (unstrided) resources: the range check is on the byte offset alone
__device__ __forceinline__ __amdgpu_buffer_rsrc_t bytes_rsrc(const void* p, int bytes) {
    return __builtin_amdgcn_make_buffer_rsrc((void*)p, (short)0, bytes, 0x00020000);
}
__device__ __forceinline__ __amdgpu_buffer_rsrc_t plane_rsrc(const float* p, int bytes) { return bytes_rsrc(p, bytes); }

__device__ __forceinline__ float ld_f32(__amdgpu_buffer_rsrc_t r, unsigned off) {
    return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, off, 0, 0));
}
__device__ __forceinline__ unsigned ld_u8(__amdgpu_buffer_rsrc_t r, unsigned off) {
    return __builtin_amdgcn_raw_buffer_load_b8(r, off, 0, 0);
}

// four consecutive fp32 of a row, the first at byte offset off; in_row and n as above
__device__ __forceinline__ f4 load4_f32(__amdgpu_buffer_rsrc_t r, bool wide, bool in_row, int n, unsigned off) {
    if (wide && (!in_row || n == 4 || n <= 0))
        return __builtin_bit_cast(f4, __builtin_amdgcn_raw_buffer_load_b128(r, in_row && n == 4 ? off : kOOB, 0, 0));
    f4 v;
    v.x = ld_f32(r, in_row && n > 0 ? off : kOOB);
    v.y = ld_f32(r, in_row && n > 1 ? off + 4u : kOOB);
    v.z = ld_f32(r, in_row && n > 2 ? off + 8u : kOOB);
    v.w = ld_f32(r, in_row && n > 3 ? off + 12u : kOOB);
    return v;
}

// four interleaved 3-byte pixels of a row as three dwords (byte q = channel q % 3 of pixel q / 3)
__device__ __forceinline__ void load4_rgb8(__amdgpu_buffer_rsrc_t r, bool wide, bool in_row, int n, unsigned off,
                                           unsigned (&d)[3]) {
    typedef unsigned u32x3 __attribute__((ext_vector_type(3)));
    if (wide && (!in_row || n == 4 || n <= 0)) {
        const u32x3 v = __builtin_amdgcn_raw_buffer_load_b96(r, in_row && n == 4 ? off : kOOB, 0, 0);
        d[0] = v.x, d[1] = v.y, d[2] = v.z;
        return;
    }
    d[0] = d[1] = d[2] = 0u;
#pragma unroll
    for (int q = 0; q < 12; ++q) d[q >> 2] |= (ld_u8(r, in_row && q < 3 * n ? off + q : kOOB) & 0xffu) << ((q & 3) * 8);
}

// n (0..4) leading values of v to p[0..n): one 128-bit store where p is 16-byte aligned
__device__ __forceinline__ void store4_f32(float* p, f4 v, int n) {
    if (n == 4 && ((size_t)p & 15) == 0) {
        *(f4*)p = v;
        return;
    }
    if (n > 0) p[0] = v.x;
    if (n > 1) p[1] = v.y;
    if (n > 2) p[2] = v.z;
    if (n > 3) p[3] = v.w;
}

namespace nconv {

// A batch of B planes of H rows; checked and filled by view_args in capi_common.h. Strides are in the
// unit the owning struct states.
struct PlaneView {
    const void* base;
    long long bs;  // image stride; 0 where B == 1
    long long rs;  // row stride
    int wide;      // base and strides keep every group of four pixels aligned for the wide loads
    template <typename T>
    __host__ __device__ const T* image(int b) const {
        return (const T*)base + (long long)b * bs;
    }
};

// The pixel-tile grid: a plane is cut into tiles of TH x TW pixels, row-major; a 1-D grid takes the
// tiles of image 0, then image 1, ..: one workgroup per tile.
template <int TH, int TW>
__host__ __device__ __forceinline__ int tiles_per_image(int H, int W) {
    return ((H + TH - 1) / TH) * ((W + TW - 1) / TW);
}
// first row and column of tile t of an image
template <int TH, int TW>
__device__ __forceinline__ void tile_corner(int W, int t, int& i0, int& j0) {
    const int ntw = (W + TW - 1) / TW;
    i0 = (t / ntw) * TH, j0 = (t % ntw) * TW;
}
struct TileOrigin {
    int b, i0, j0;  // image; the tile's first row and column
};
// the tile of this workgroup
template <int TH, int TW>
__device__ __forceinline__ TileOrigin tile_origin(int H, int W) {
    const int per = tiles_per_image<TH, TW>(H, W);
    TileOrigin o;
    o.b = blockIdx.x / per;
    tile_corner<TH, TW>(W, blockIdx.x - o.b * per, o.i0, o.j0);
    return o;
}

// The 16 x 64 tile of the loss family (loss.hip, conf_loss.hip, metrics.hip, view_warp.hip, smooth_loss.hip): 1024
// pixels, four per thread of a 256-thread workgroup.
constexpr int kLossTH = 16, kLossTW = 64;
__host__ __device__ __forceinline__ int loss_tiles_per_image(int H, int W) {
    return tiles_per_image<kLossTH, kLossTW>(H, W);
}

// That tile with four consecutive pixels of a row per thread (conf_loss.hip, metrics.hip): thread t
// owns row t >> 4, columns 4 (t & 15) .. + 3.
struct Quad {
    int b, i, j, n;  // image; the thread's row and first column; how many of its four pixels are in the row
    bool row_in;
};
__device__ __forceinline__ Quad loss_quad(int H, int W) {
    const TileOrigin o = tile_origin<kLossTH, kLossTW>(H, W);
    Quad q;
    q.b = o.b;
    q.i = o.i0 + (threadIdx.x >> 4);
    q.j = o.j0 + (threadIdx.x & 15) * 4;
    q.row_in = q.i < H;
    q.n = min(4, W - q.j);
    return q;
}
// the thread's four pixels of an fp32 view (strides in elements); pixels outside the plane read 0
using ::load4_f32;
__device__ __forceinline__ f4 load4_f32(const PlaneView& p, int H, int W, const Quad& q) {
    const __amdgpu_buffer_rsrc_t rs = plane_rsrc(p.image<float>(q.b), view_bytes(H, p.rs, W, 4));
    return load4_f32(rs, p.wide != 0, q.row_in, q.n, (unsigned)((long long)q.i * p.rs + q.j) * 4u);
}

}  // namespace nconv
