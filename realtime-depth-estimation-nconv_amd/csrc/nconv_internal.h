// nconv_internal.h — launcher interface between the C-ABI layer (nconv_capi.hip, capi_dense.hip,
// capi_io.hip) and the kernel translation units. Not part of the public ABI.
#pragma once
#include "nconv_common.h"

namespace nconv {

// after the launches of a host function: 0, or -EIO with *why = the runtime's message
inline int launch_status(const char** why) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        *why = hipGetErrorString(e);
        return -5;
    }
    return 0;
}

struct TailArgs {
    const float* w7;
    const float* b7;
    const float* s7;
    float eps7;
    int off;
    int out_h, out_w;
    float* out_c;
    float* py;  // optional 2x2 max-pooled copies of y / cout (non-tail launches), (B,Cout,Ho/2,Wo/2)
    float* pc;
    unsigned* parg;  // optional (with py): per pooled element the two first-maximum slots
    // fused head (nconv_fwd_head): nconv1 evaluated while staging nconv2's input
    const float* s_in;  // sparse depth (B, 1, H, W)
    const float* w1;    // nconv1 weight (8, 1, 5, 5), bias, s[o]
    const float* b1;
    const float* s1;
    float eps1, thresh1;
    float* y1;  // optional (training): nconv1's outputs (B, 8, H, W) written by the fused head
    float* c1;
    float* y6;  // optional (training): nconv6's outputs written by the fused tail (phase kernel)
    float* c6;
};

struct BwdArgs {
    const float* y;
    const float* co;
    const float* gy;
    const float* gco;  // may be null (= 0)
    float* gxa;
    float* gca;
    float* gxb;
    float* gcb;
    float* gw;
    float* gb;
    float* ws;  // workspace
    size_t ws_bytes;
    int accumulate;  // 1: += into gxa/gca/gxb/gcb; 0: overwrite every element
    int defer;       // 1: leave the weight gradient as partial rows (reduced by launch_wgrad_reduce_multi)
    int* nparts;     // out (defer): the number of partial rows written
    // optional: gradient of the 2x2 max-pooled outputs (B, Cout, Ho/2, Wo/2) and the pooling argmax
    // codes (nconv_fwd_pooled), routed into gy / gcout while {gN, gD} are formed (pool_route)
    const float* gpy;
    const float* gpc;
    const unsigned* parg;
    // optional fused weight gradient of the producer nconv1 (1 -> 8, 5x5, threshold load, padding 2)
    // in the input gradient's epilogue: its sparse input S, bias, normaliser, eps, threshold, and
    // the per-workgroup partial rows (200 weights, 8 sum gy, 8 sum gcout*cout) it writes
    const float* hS;
    const float* hb;
    const float* hs;
    float heps, hthresh;
    float* hpart;
    float* hgw;       // nconv1's gW / gb (undeferred: reduced right after the kernel)
    float* hgb;
    int* hnparts;     // out (defer): the number of nconv1 partial rows written
    // optional fused backward of the consumer nconv7 (8 -> 1, 1x1, padding 2) of this layer's
    // outputs: gy / gco of this layer are formed from nconv7's (gy, y, cout) planes (B, 1, Ho + 4,
    // Wo + 4) and its weights; nconv7's weight gradient goes to t7part (10-float partial rows)
    const float* t7w;
    const float* t7b;
    const float* t7s;
    float t7eps;
    const float* t7gy;
    const float* t7y;
    const float* t7co;
    float* t7part;
    float* t7gw;
    int* t7nparts;
    int t7ph, t7pw, t7pc0;  // nconv7's planes: (t7ph, t7pw) holding its grid from row / column t7pc0
    const float* box;  // optional precomputed box weights of an exactly-2x UPCAT layer (dgrad_phase)
    // nconv7's cout gradient (nconv_bwd_tail_conf), the same planes as t7gy; null: 0. Last, so that the
    // kernel-argument offsets of the fields above stay as they were.
    const float* t7gco;
};
// nconv7 (1x1, padding 2) consumer fused into its producer's backward (T7): byte offset of nconv6
// pixel (oh, ow) in nconv7's planes -- its (Ho + 4) x (Wo + 4) grid, or the window of it that DNET's
// crop keeps (t7ph x t7pw from row / column t7pc0) -- or oob outside nconv6's grid or the window (a
// zero gradient there); nconv7's {gN7, gD7} from its (gy, gcout, y, cout) (gcout: 0 without t7gco);
// nconv6's (gy, gcout) from them and w7[o] as nconv7's own 1x1 input gradient forms them
// (dgrad_tiled<8,1,1>'s epilogue, same operations)
__device__ __forceinline__ unsigned t7_off(const BwdArgs& a, int oh, int ow, int Ho, int Wo, unsigned oob) {
    const int r = oh + 2 - a.t7pc0, c = ow + 2 - a.t7pc0;
    return ((unsigned)oh < (unsigned)Ho && (unsigned)ow < (unsigned)Wo && (unsigned)r < (unsigned)a.t7ph &&
            (unsigned)c < (unsigned)a.t7pw)
               ? (unsigned)(r * a.t7pw + c) * 4u
               : oob;
}
__device__ __forceinline__ void t7_nd(const BwdArgs& a, float gy9, float gco9, float y9, float co9, float& gN7,
                                      float& gD7) {
    nconv_grad_nd(gy9, gco9, y9, co9, a.t7eps, a.t7b[0], a.t7s[0], gN7, gD7);
}
__device__ __forceinline__ void t7_gy(float w7, float gN7, float gD7, float y, float co, float& gy, float& gco) {
    const float gxc = fmaf(w7, gN7, 0.f), gc = fmaf(w7, gD7, 0.f);  // the 1x1 dgrad's accumulators
    gy = gxc * co;
    gco = fmaf(gxc, y, gc);
}
size_t bwd_tail_workspace_bytes(const nconv_layer& L6);
size_t bwd_head_workspace_bytes(const nconv_layer& L2);

// One layer's deferred weight-gradient reduction (nconv_wgrad_reduce): its workspace's partial rows.
struct RedJob {
    const float* part;  // nblk partial rows of nw + 2 cout floats, then the kReduceSplit slice rows
    const float* wsum;
    float* gw;
    float* gb;
    int nblk, nw, cout, fan;
    // flat (nconv_wgrad_reduce_ex sums): gb[0] = the sum of part[0 .. nblk) (nw = 0, cout = 1) in a
    // fixed order -- kSumChunks chunk sums into sub, then their tree
    int flat;
    float* sub;
};
constexpr int kMaxRedJobs = 16;
constexpr int kSumChunks = 1024;
constexpr int kReduceSplit = 16;  // slice-sum rows after a layer's partial rows (nconv_wgrad.hip)
int launch_wgrad_reduce_multi(int n, const RedJob* jobs, hipStream_t st, const char** why);
// one layer's nblk partial rows at part: reduced into a.gw / a.gb now, or (a.defer) left for a later
// nconv_wgrad_reduce with *a.nparts = nblk
int launch_wgrad_reduce(const BwdArgs& a, const float* part, int nblk, int nw, int cout, int fan,
                        const float* wsum, hipStream_t st, const char** why);

// Forward. Return 0, or a negative errno with *why set.
int launch_fwd(const LayerDev& d, float* y, float* yc, float* py, float* pc, unsigned* parg, hipStream_t st,
               const char** why);
bool fwd_mfma_supported(const nconv_layer& L, bool tail, bool pool);
bool launch_fwd_mfma(const LayerDev& d, float* y, float* yc, const TailArgs& t, bool tail, hipStream_t st);
// exact-fp32 UPCAT layers with the upsampled half at native resolution (nconv_fwd_phase.hip)
bool fwd_phase_supported(const nconv_layer& L, bool tail);
bool launch_fwd_phase(const LayerDev& d, float* y, float* yc, const TailArgs& t, bool tail, hipStream_t st);
size_t phase_weight_floats(const nconv_layer& L);
int launch_phase_weights(int n, const float* const* w, const int* cin, const int* up_first, float* const* out,
                         hipStream_t st, const char** why);
// enum nconv_kernel of the forward / input-gradient / weight-gradient launches (nconv_plan)
int plan_fwd(const nconv_layer& L);
void plan_bwd(const nconv_layer& L, int* dgrad, int* wgrad);
int launch_fwd_head(const LayerDev& d2, const TailArgs& t, float* y, float* yc, hipStream_t st, const char** why);
// exact-fp32 fused head (nconv_fwd_head.hip); d2.L.waux = the composed confidence weights
int launch_fwd_head_exact(const LayerDev& d2, const TailArgs& t, float* y, float* yc, hipStream_t st,
                          const char** why);
int launch_weight_prologue(int n, float* const* w, const int* cout, const int* fan_in, float* const* s,
                           const float* w1, const float* w2, float* w21, int nphase, const float* const* pw,
                           const int* pcin, const int* pup_first, float* const* pout, hipStream_t st,
                           const char** why);
int launch_train_prologue(int n, float* const* w, const int* cout, const int* fan_in, const int* sp,
                          float* const* s, int head1, int head2, float* w21, unsigned* sync, int nphase,
                          const int* players, const int* pup_first, float* const* pout, float* const* pbox,
                          hipStream_t st, const char** why);
int launch_head_weights(const float* w1, const float* s1, const float* w2, float* out, hipStream_t st,
                        const char** why);
int launch_fwd_tail(const LayerDev& d, const TailArgs& t, float* out, hipStream_t st, const char** why);
int launch_weight_prep(int n, float* const* w, const int* cout, const int* fan_in, const int* sp,
                       float* const* s, hipStream_t st, const char** why);

// Grid sizing (nconv_occ.hip): CUs of the current device, resident workgroups per CU of a kernel
// on it (>= 1); cached per device ordinal, thread-safe.
int dev_cus();
int dev_occupancy(const void* kernel, int threads, size_t dyn_lds);

// Backward.
inline bool is_upcat(const nconv_layer& L) {
    return L.load_mode == NCONV_LOAD_UPCAT_SKIP_FIRST || L.load_mode == NCONV_LOAD_UPCAT_UP_FIRST;
}
size_t bwd_workspace_bytes(const LayerDev& d);
// weight gradient on the bf16 matrix cores (nconv_wgrad_bf.hip): np = 2 (bf16x3) or 3 (bf16x9) split
// parts; at most max_blocks partial rows into part; returns the number written
template <int CIN, int COUT, int K, int MODE>
int go_wgrad_bf(const LayerDev& d, const BwdArgs& a, float* part, int max_blocks, int np, hipStream_t st);
// input gradient on the bf16 matrix cores (nconv_dgrad_bf.hip), np as go_wgrad_bf
template <int CIN, int COUT, int K, int MODE>
void go_dgrad_bf(const LayerDev& d, const BwdArgs& a, float* tmp_x, float* tmp_c, int np, hipStream_t st);
// exact-fp32 input gradient (nconv_dgrad.hip): dgrad_tiled, or dgrad_phase where dgrad_phase_ok(L);
// GP: pooled-gradient routing, HW: fused nconv1 weight gradient (its partial rows reduced or, with
// a.defer, counted in *a.hnparts), T7: fused nconv7 backward. tx / tc: the staged upsampled planes.
bool dgrad_phase_ok(const nconv_layer& L);
size_t dgrad_blocks(const nconv_layer& L);  // workgroups of the tiled / phase input gradient
template <int CIN, int COUT, int K, int MODE, bool GP, bool HW, bool T7>
int go_dgrad(const LayerDev& d, const BwdArgs& a, float* tx, float* tc, hipStream_t st, const char** why);
int launch_dgrad_generic(const LayerDev& d, const BwdArgs& a, float* tx, float* tc, hipStream_t st,
                         const char** why);
void launch_upsample_bwd_gather(const LayerDev& d, const BwdArgs& a, const float* tx, const float* tc,
                                hipStream_t st);
// exact-fp32 weight-gradient partial rows into part, returning their number: wgrad_tiled (<=
// max_blocks); wgrad_mfma / wgrad_mfma2 (<= wgrad_mfma_max_blocks; T7: nconv7's rows to a.t7part too)
template <int CIN, int COUT, int K, int MODE>
int go_wgrad_tiled(const LayerDev& d, const BwdArgs& a, float* part, int max_blocks, hipStream_t st);
template <int CIN, int COUT, int K, int MODE, bool GP, bool T7>
int go_wgrad_mfma(const LayerDev& d, const BwdArgs& a, float* part, hipStream_t st);
size_t wgrad_mfma_max_blocks(const nconv_layer& L);
int launch_wgrad_generic(const LayerDev& d, const BwdArgs& a, float* part, int nchunk, hipStream_t st,
                         const char** why);
int launch_bwd(const LayerDev& d, const BwdArgs& a, hipStream_t st, const char** why);
// nconv1's weight-gradient partial rows of the fused head (200 weights, 8 sum gy, 8 sum gcout*cout)
constexpr int kHeadNw = 8 * 25, kHeadStride = kHeadNw + 16;
// Dense convolutions (RGB-guided model).
int dense_cout_tile(int Cout);
size_t dense_packed_floats(int kind, int Cin, int Cout);
int launch_dense_pack(int kind, int Cin, int Cout, const float* w, const float* scale, float* wp, hipStream_t st,
                      const char** why);
int launch_dense_conv(const nconv_dense_conv& p, hipStream_t st, const char** why);
int launch_bilinear_ac(const float* x, int B, int C, int H, int W, float* y, int Ho, int Wo, hipStream_t st,
                       const char** why);
int launch_conv3x3_c1(const float* x, int B, int Cin, int H, int W, const float* w, const float* res, float* out,
                      hipStream_t st, const char** why);
size_t dense_wgrad_workspace_bytes(const nconv_dense_wgrad& g);
int launch_dense_wgrad(const nconv_dense_wgrad& g, float* ws, size_t ws_bytes, hipStream_t st, const char** why);

// Training-mode BatchNorm (+ ReLU).
size_t bn_workspace_bytes(const nconv_bn_train& p);
int launch_bn_train_fwd(const nconv_bn_train& p, float* ws, hipStream_t st, const char** why);
size_t relu_bias_workspace_bytes(int B, int C, int H, int W);
int launch_relu_bias_bwd(int B, int C, int H, int W, const float* g, const float* out, float* gm, float* gbias,
                         float* ws, hipStream_t st, const char** why);
int launch_bn_train_bwd(const nconv_bn_train& p, const float* gy, float* gx, float* ggamma, float* gbeta, float* ws,
                        hipStream_t st, const char** why);

// Training loss (utils.py calculate_loss) on B planes.
struct LossArgs {
    PlaneView r, t;  // fp32, strides in elements (wide is not used: the loss reads halo windows)
    int B, H, W;
};
size_t loss_workspace_bytes(int B, int H, int W);
int launch_loss_fwd(const LossArgs& a, int grad_loss, float* loss, float* ws, hipStream_t st, const char** why);
int launch_loss_bwd(const LossArgs& a, int grad_loss, const float* gout, const float* ws, float* g, hipStream_t st,
                    const char** why);

// Confidence loss (nconv_conf_loss_fwd / _bwd, conf_loss.hip) on B planes.
struct ConfLossArgs {
    PlaneView r, c, t;  // prediction, confidence, target: fp32, strides in elements; wide: 16-byte aligned
                        // base and strides, four pixels of a row then come in one load (plane_io.h)
    int B, H, W;
    int kind;           // enum nconv_conf_loss_err
    float beta;
    const float* lam;   // device scalar
};
size_t conf_loss_workspace_bytes(int B, int H, int W);
int launch_conf_loss_fwd(const ConfLossArgs& a, float* loss, void* ws, hipStream_t st, const char** why);
int launch_conf_loss_bwd(const ConfLossArgs& a, const float* gloss, float* g_r, float* g_c, hipStream_t st,
                         const char** why);

// Evaluation metrics (the twelve raw sums of nconv_depth_metrics) on B planes.
struct MetricsArgs {
    PlaneView p, g;     // prediction and target: fp32, strides in elements
    int B, H, W;
    float g_lo, g_hi;   // validity window of the target (absent bounds: 0, +inf)
    float c_lo, c_hi;   // clamp window of the prediction (absent bounds: -inf, +inf)
};
size_t metrics_workspace_bytes(int B, int H, int W);
int launch_metrics(const MetricsArgs& a, double* sums, double* accum, void* ws, hipStream_t st, const char** why);

// Raw frame ingest (nconv_frame_ingest) and 16-bit depth export (nconv_depth_export_u16), frame_io.hip.
struct IngestPlane {
    PlaneView src;     // base null: absent; strides in bytes; wide: 4-byte aligned (F32: 16-byte)
    float* out;        // (B, 1, h, w) contiguous
    int dtype, shift;  // enum nconv_frame_dtype; right shift of the integer value
    float scale;
};
struct IngestArgs {
    int B, h, w;
    int reverse;     // RGB planes written in reverse channel order
    PlaneView rgb;   // base null: absent; uint8 interleaved, strides in bytes; wide: 4-byte aligned
    float* rgb_out;  // (B, 3, h, w) contiguous
    IngestPlane pl[2];
};
int launch_frame_ingest(const IngestArgs& a, hipStream_t st, const char** why);

struct ExportArgs {
    PlaneView d;  // fp32, strides in elements
    int B, H, W;
    float scale;
    unsigned short* out;  // (B, 1, H, W) contiguous
};
int launch_depth_export(const ExportArgs& a, hipStream_t st, const char** why);

// Back-projection of a depth map to 3-D points (nconv_backproject_map / _points), backproject.hip.
struct BackprojectArgs {
    int B, H, W;
    int nseg;                // B * H * ceil(W / 256) segments of 256 row pixels, one wave each
    PlaneView depth;         // fp32, strides in elements
    PlaneView conf;          // base null: no confidence gate; fp32, strides in elements
    PlaneView color;         // base null: none; else per color_kind, strides in elements of its type
    int color_kind, reverse;
    long long ocs;           // channel stride of a planar colour (elements)
    const float* k;
    long long kbs;           // image stride of K in floats (0: one camera)
    float z_min, z_max, conf_min;
};
long long backproject_segments(int B, int H, int W);
size_t backproject_workspace_bytes(int B, int H, int W);
int launch_backproject_map(const BackprojectArgs& a, float* xyz, hipStream_t st, const char** why);
int launch_backproject_points(const BackprojectArgs& a, float* xyz, unsigned char* rgb, int* index, int capacity,
                              int* offsets, int* ws, hipStream_t st, const char** why);

// Surface normals of a depth map (nconv_depth_normals / _points), normals.hip; the sources are a
// BackprojectArgs (its colour is not read).
struct NormalsArgs {
    float jump_rel, jump_abs;  // a neighbour is usable within jump_abs + jump_rel * z of the centre's depth
    int gate;                  // 0: both are 0, every valid neighbour is usable
    unsigned empty;            // the picture's pixel without a normal: R | G << 8 | B << 16
};
int launch_depth_normals(const BackprojectArgs& a, const NormalsArgs& o, float* normals, unsigned char* image,
                         hipStream_t st, const char** why);
int launch_depth_normals_points(const BackprojectArgs& a, const NormalsArgs& o, const int* index, const int* offsets,
                                int capacity, float* normals, hipStream_t st, const char** why);

// Projection of a LiDAR scan to the sparse depth plane (nconv_lidar_project), lidar_project.hip.
struct LidarArgs {
    int B, H, W;
    int n_rows;            // rows of points (< 2^31)
    int stride;            // floats per row (3 .. 2^20)
    int vec;               // stride == 4 and a 16-byte aligned base: 128-bit row loads
    const float* points;
    const int* offsets;    // (B + 1), on the device
    const float* m;
    long long mbs;         // image stride of m in floats (0: one camera)
    float z_min, z_max;
};
// keys: null = the 32-bit z-buffer in `depth` itself; else B * H * W 64-bit keys (index is written too)
int launch_lidar_project(const LidarArgs& a, float* depth, int* index, unsigned long long* keys, hipStream_t st,
                         const char** why);

// Depth plane -> colour image (nconv_depth_colorize), colorize.hip.
struct ColorizeArgs {
    PlaneView d;               // fp32, strides in elements
    PlaneView bg;              // base null: none; uint8 interleaved, strides in bytes; wide: 4-byte aligned
    int B, H, W;
    const unsigned char* lut;  // 256 x 3 RGB on the device, or null: the builtin table cmap
    int cmap;
    int auto_range;            // lo / hi from range[2 b], range[2 b + 1] (order-preserving keys)
    int radius, bgr;
    float lo, hi, floor;
    unsigned empty;            // the colour of an empty pixel, packed as the table entries are
    unsigned char* out;        // (B, H, W, 3) contiguous
    unsigned* range;           // 2 * B keys (auto_range)
};
int launch_depth_colorize(const ColorizeArgs& a, hipStream_t st, const char** why);

// Exact-count random subset of a depth plane (nconv_depth_sparsify), sparsify.hip.
struct SparsifySel {
    unsigned long long prefix;  // the digits of the threshold key resolved so far, from the top
    unsigned rank;              // 0-based rank of the threshold among the candidates under that prefix
    int n;                      // n_b
};
struct SparsifyArgs {
    int B, H, W;
    int mode;                     // enum nconv_sparsify_mode
    const float* src;             // strides in elements (64-bit offsets: no limit on the extent)
    long long sbs, srs;
    const unsigned char* mask;    // null: none; strides in bytes, mbs 0: one mask for the batch
    long long mbs, mrs;
    const unsigned* state;        // seed_lo, seed_hi, draw
    const int* n_dev;
    int n;
    float keep;
    int all_pixels;
    float floor;
    unsigned key_mask, noise_threshold;
    float noise_amp;
    float* dst;                   // may be src with the same strides
    long long dbs, drs;
    int* kept;                    // null: skip
    unsigned* hist;               // [pass][image][bin]
    SparsifySel* sel;             // [pass][image]
};
size_t sparsify_workspace_bytes(int B);
int launch_depth_sparsify(SparsifyArgs a, void* workspace, hipStream_t st, const char** why);

// Occluded LiDAR returns removed from a sparse depth plane (nconv_depth_occlusion), occlusion.hip.
struct OcclusionArgs {
    PlaneView s;              // fp32, strides in elements
    int B, H, W;
    int rh, rw;               // 0 .. 16
    int min_support;
    float jump_abs, jump_rel, floor;
    float* dst;               // strides in elements; disjoint from the source
    long long dbs, drs;
    unsigned char* removed;   // (B, H, W) contiguous, or null
    int* index;               // (B, H, W) contiguous, updated in place, or null
    int* counts;              // (B, 2), or null
};
int launch_depth_occlusion(const OcclusionArgs& a, hipStream_t st, const char** why);

// Random crop, flip and colour jitter of a training batch (nconv_frame_augment), augment.hip.
enum SlotKind { kPlane = 0, kRgb = 1, kMask = 2 };
struct AugmentSlot {
    const void* src;   // image 0 (of this channel)
    void* dst;
    long long bs, rs;  // source strides: elements (bytes for the mask); bs 0 where B == 1
    long long dbs;     // output image stride in elements
    int kind, chan;
};
constexpr int kMaxSlots = 7;  // three RGB channels, three planes, the mask
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
int launch_frame_augment(const AugmentArgs& a, hipStream_t st, const char** why);

// Sparsification curves of a confidence plane (nconv_depth_sparsification), sparsification.hip.
struct SparsificationArgs {
    PlaneView p, g, c;  // prediction, target, confidence: fp32, strides in elements (wide is not used)
    int B, H, W;
    float g_lo, g_hi;   // validity window of the target (absent bounds: 0, +inf)
    float c_lo, c_hi;   // clamp window of the prediction (absent bounds: -inf, +inf)
    int steps;          // J
    int uncertainty;    // the plane is an uncertainty: larger is removed first
    double* curves;     // (B, 2, J, 3)
    int* order;         // (B, 2, H * W); null: skip
};
size_t sparsification_workspace_bytes(int B, int H, int W);
int launch_depth_sparsification(const SparsificationArgs& a, void* workspace, hipStream_t st, const char** why);

// Classical depth completion of a sparse plane, IP-Basic (nconv_depth_ipbasic), ipbasic.hip.
struct IpbasicArgs {
    PlaneView s;              // fp32, strides in elements
    int B, H, W;
    float max_depth;
    int shape, r1;            // enum nconv_ipbasic_kernel; the custom kernel's radius 1 .. 3
    int extrapolate, median, blur, keep_samples;
    float* dst;               // strides in elements; disjoint from the source
    long long dbs, drs;
    float* work;              // (B, H, W) contiguous: v3 (extrapolate)
    int* top;                 // (B, W): top(x), INT_MAX where the column has no valid pixel (extrapolate)
};
int launch_depth_ipbasic(const IpbasicArgs& a, hipStream_t st, const char** why);

// Nearest sample and distance map of a sparse depth plane (nconv_depth_nearest), nearest.hip.
struct NearestArgs {
    PlaneView s;              // fp32, strides in elements (wide is not used: single pixels are read)
    int B, H, W;
    float floor;
    int max_dist2;            // < 0: no limit
    float* dst;               // strides in elements; disjoint from the source; or null
    long long dbs, drs;
    int* index;               // (B, H, W) contiguous, or null
    int* dist2;               // (B, H, W) contiguous, or null
    float* dist;              // (B, H, W) contiguous, or null
    int* work;                // (B, H, W) contiguous: the row of each column's nearest sample, -1: none
};
int launch_depth_nearest(const NearestArgs& a, hipStream_t st, const char** why);

// Depth-driven view warp and photometric loss (nconv_view_warp_*, nconv_photo_loss_*), view_warp.hip.
struct WarpArgs {
    int B, C, H, W, Hs, Ws;   // target planes (H, W), source planes (Hs, Ws), C = 1 or 3
    PlaneView depth;          // fp32 (B, H, W), strides in elements (wide is not used: one pixel per lane)
    PlaneView mask;           // base null: none; uint8 (B, H, W), strides in bytes; bs 0: one mask for the batch
    PlaneView src;            // fp32 (B, C, Hs, Ws); rs / bs of one channel plane, channels scs apart
    long long scs;
    PlaneView tgt;            // base null: the plain warp; fp32 (B, C, H, W), channels tcs apart
    long long tcs;
    const float* k;
    long long kbs;            // image stride of K in floats (0: one camera)
    const float* m;
    long long mbs;            // image stride of m in floats (0: one matrix)
    float z_min, z_max;
};
size_t photo_loss_workspace_bytes(int B, int H, int W);
int launch_view_warp_fwd(const WarpArgs& a, float* warped, unsigned char* valid, hipStream_t st, const char** why);
int launch_view_warp_bwd(const WarpArgs& a, const float* g_warped, float* g_depth, hipStream_t st, const char** why);
int launch_photo_loss_fwd(const WarpArgs& a, float* loss, void* ws, hipStream_t st, const char** why);
int launch_photo_loss_bwd(const WarpArgs& a, const float* gloss, const void* ws, float* g_depth, hipStream_t st,
                          const char** why);
// The same loss with the SSIM term over 3 x 3 windows (nconv_photo_ssim_loss_*), photo_ssim.hip.
size_t photo_ssim_workspace_bytes(int B, int H, int W);
int launch_photo_ssim_loss_fwd(const WarpArgs& a, float alpha, float c1, float c2, float* loss, void* ws,
                               hipStream_t st, const char** why);
int launch_photo_ssim_loss_bwd(const WarpArgs& a, float alpha, float c1, float c2, const float* gloss, const void* ws,
                               float* g_depth, hipStream_t st, const char** why);
// The minimum of that loss's per-pixel error over several sources, with auto-masking
// (nconv_photo_min_loss_*), photo_min.hip.
constexpr int kMinSources = 4;
struct MinArgs {
    WarpArgs v[kMinSources];  // the S sources with tgt; they differ in src, scs, Hs, Ws, m and mbs alone
    int S, automask;          // automask 0 / 1; 1 needs Hs == H and Ws == W for every source
    float alpha, c1, c2;
};
size_t photo_min_workspace_bytes(int B, int H, int W);
int launch_photo_min_loss_fwd(const MinArgs& m, float* loss, unsigned char* winner, float* error, void* ws,
                              hipStream_t st, const char** why);
int launch_photo_min_loss_bwd(const MinArgs& m, const float* gloss, const void* ws, float* g_depth, hipStream_t st,
                              const char** why);

// Cross-view depth consistency: the check with fusion and the geometry-consistency loss
// (nconv_depth_consistency, nconv_geo_consistency_loss_*), consistency.hip.
struct ConsistencyArgs {
    WarpArgs v[kMinSources];          // the S sources, src = the source's depth plane (C == 1); they differ in
                                      // src, Hs, Ws, m and mbs alone
    const float* k_src[kMinSources];  // 3 x 3 of the source camera, images ksbs floats apart (0: one camera)
    long long ksbs[kMinSources];
    const float* m_back[kMinSources]; // 3 x 4, K_tgt . [R | t]^-1, images mbbs floats apart (0: one matrix)
    long long mbbs[kMinSources];
    int S, min_views;
    float px_tol, rel_tol;
};
size_t geo_consistency_workspace_bytes(int B, int H, int W);
int launch_depth_consistency(const ConsistencyArgs& m, float* fused, unsigned char* count, unsigned char* views,
                             float* reproj, float* reldiff, hipStream_t st, const char** why);
int launch_geo_consistency_loss_fwd(const WarpArgs& a, float* loss, float* diff, void* ws, hipStream_t st,
                                    const char** why);
int launch_geo_consistency_loss_bwd(const WarpArgs& a, const float* gloss, const void* ws, float* g_depth,
                                    hipStream_t st, const char** why);

// Relative pose by direct image alignment (nconv_pose_normal_eq, nconv_pose_update), pose_align.hip.
constexpr int kPoseSums = 28;  // 21 of the upper triangle of sum w J^T J, 6 of sum w J r, sum w r^2
struct PoseArgs {
    WarpArgs w;               // the warp's operands with tgt; w.m is the fp32 m that the update rewrites
    const float* k_src;
    long long ksbs;           // image stride of K_src in floats (0: one camera)
    float* pose;              // fp32 (B, 3, 4) contiguous: read by normal_eq, rewritten by the update
    float* m_out;             // w.m as the update writes it
    float huber, damping;
    int min_points;
    int* status;              // (B)
    float* cost;              // (B, history)
    int* n;                   // (B, history)
    int history;
};
size_t pose_workspace_bytes(int B, int H, int W);
int launch_pose_normal_eq(const PoseArgs& a, void* ws, hipStream_t st, const char** why);
int launch_pose_update(const PoseArgs& a, void* ws, int it, int apply, hipStream_t st, const char** why);

// Edge-aware depth smoothness loss and the edge weights (nconv_smooth_loss_*, nconv_edge_weights), smooth_loss.hip.
struct SmoothArgs {
    int B, H, W, order;       // order 1: first differences, 2: second differences
    PlaneView depth;          // fp32 (B, H, W), strides in elements (wide is not used: one pixel per lane)
    PlaneView mask;           // base null: none; uint8 (B, H, W), strides in bytes
    const float* w;           // null: every weight 1; fp32 (B, 2, H, W) contiguous, wx then wy
};
size_t smooth_loss_workspace_bytes(int B, int H, int W);
int launch_smooth_loss_fwd(const SmoothArgs& a, float* loss, void* ws, hipStream_t st, const char** why);
int launch_smooth_loss_bwd(const SmoothArgs& a, const float* gloss, const void* ws, float* g_depth, hipStream_t st,
                           const char** why);
struct EdgeArgs {
    int B, C, H, W;           // C = 1 or 3
    PlaneView img;            // fp32 (B, C, H, W); rs / bs of one channel plane, channels cs apart
    long long cs;
    float alpha;
};
int launch_edge_weights(const EdgeArgs& a, float* w, hipStream_t st, const char** why);

// Voxel-grid merge of point clouds (nconv_voxel_merge), voxel_merge.hip.
struct VoxelArgs {
    long long N;                 // rows of the inputs, 0 <= N < 2^31
    const float* xyz;            // (N, 3) fp32, rows xs floats apart
    long long xs;
    const unsigned char* rgb;    // null: none; (N, 3) uint8, rows cs bytes apart
    long long cs;
    const float* nrm;            // null: none; (N, 3) fp32, rows ns floats apart
    long long ns;
    const int* w;                // null: every weight 1; (N)
    const int* offsets;          // null: one segment of all rows; (S + 1)
    const float* poses;          // null: identity; (S, 3, 4) contiguous
    int S, nx, ny, nz;
    float voxel, ox, oy, oz;
    long long cap;               // rows of the outputs
    float* oxyz;                 // (cap, 3)
    unsigned char* orgb;         // (cap, 3), with rgb
    float* onrm;                 // (cap, 3), with nrm
    int *ocount, *okey;          // (cap)
    int* stats;                  // (4)
};
size_t voxel_merge_workspace_bytes(long long N);
int launch_voxel_merge(const VoxelArgs& a, void* ws, hipStream_t st, const char** why);

}  // namespace nconv
