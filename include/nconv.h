/*
 * nconv.h — C ABI of libnconv.so, the MI355X (gfx950) normalized-convolution library.
 *
 * The reference (lllllcf/Realtime-Depth-Estimation-Nconv) has no native code: its boundary is the
 * PyTorch nn.Module API of models/step1.py. Each entry point below replaces a specific group of
 * PyTorch ops the reference issues on its hot path; the replaced file:line is cited per function.
 * The Python host layer (realtime-depth-estimation-nconv_amd/) binds these with ctypes; see
 * INTEGRATION.md for the binding a maintainer of the reference would add.
 *
 * Conventions (all entry points):
 *   - every buffer is a caller-owned device pointer to contiguous fp32 NCHW memory; the library
 *     never allocates, frees or synchronises;
 *   - work is enqueued on `stream` (a hipStream_t passed as void*; NULL = the null stream);
 *   - return 0 on success or a negative errno-style code; nconv_last_error() then describes it
 *     (thread-local string, valid until the next call on the same thread);
 *   - stateless and re-entrant; safe to capture into a hipGraph (no host sync inside).
 */
#ifndef NCONV_H
#define NCONV_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NCONV_ABI_VERSION 27

/* How a layer's input (data x, confidence c) is produced from its source tensors. These are the
 * DNET glue ops fused into the layer's load stage (models/step1.py:53,61-90). */
enum nconv_load_mode {
    NCONV_LOAD_PLAIN = 0,            /* x = a.x, c = a.c                                   (step1.py:57,92)    */
    NCONV_LOAD_THRESH = 1,           /* x = a.x, c = float(a.x > thresh)                    (step1.py:53-56)    */
    NCONV_LOAD_POOL2 = 2,            /* x = maxpool2x2(a.x), c = maxpool2x2(a.c), independent (step1.py:62-75) */
    NCONV_LOAD_UPCAT_SKIP_FIRST = 3, /* x = cat(a.x, up(b.x)), c likewise                   (step1.py:78-85)    */
    NCONV_LOAD_UPCAT_UP_FIRST = 4    /* x = cat(up(b.x), a.x), c likewise                   (step1.py:88-90)    */
};

/* Arithmetic of the NConv sums (nconv_layer.math: forward N = W*(x*c), D = W*c; nconv_layer.bwd_math:
 * the backward's products). The zero value is the reference's arithmetic (F.conv2d in fp32,
 * models/step1.py:119-122), so a zero-initialised descriptor computes exact fp32. */
enum nconv_math {
    NCONV_MATH_FP32 = 0,   /* default: exact fp32 products (forward: packed FP32 FMA on the vector ALU;
                              backward: fp32 matrix cores for the weight gradient, packed FP32 for the
                              input gradient) */
    NCONV_MATH_BF16X3 = 1, /* bf16 matrix cores on split operands, v = hi + lo, products
                              hi*hi + lo*hi + hi*lo in fp32 (<= ~1.1e-5 relative per product), for
                              the 8-output-channel 5x5 (8 in) / 3x3 (16 in) layers; others FP32 */
    NCONV_MATH_BF16X9 = 2  /* exact products on the bf16 matrix cores: v = v0 + v1 + v2 and
                              w = w0 + w1 + w2 (three bf16 parts, an exact decomposition), all nine
                              partial products (each exact in fp32) accumulated in fp32, for the same
                              layers as BF16X3; others FP32 */
};

/* Kernel family a launch runs (nconv_plan). */
enum nconv_kernel {
    NCONV_KERNEL_GENERIC = 0,     /* direct one-thread-per-element kernels (any NConv2d geometry)       */
    NCONV_KERNEL_TILED_FP32 = 1,  /* LDS-tiled, exact fp32 products on the vector ALU (packed FP32)     */
    NCONV_KERNEL_MFMA_FP32 = 2,   /* fp32 matrix cores, exact fp32 products                            */
    NCONV_KERNEL_MFMA_BF16X3 = 3, /* bf16 matrix cores, two-part split operands (NCONV_MATH_BF16X3)    */
    NCONV_KERNEL_MFMA_BF16X9 = 4, /* bf16 matrix cores, three-part split, exact products (BF16X9)      */
    NCONV_KERNEL_TILED_FP32_PHASE = 5 /* as TILED_FP32, the nearest-2x-upsampled half of the input
                                     channels at native resolution: forward with phase weights
                                     (nconv_layer.waux, nconv_phase_weights); input gradient as
                                     4x4 box-summed weights per low pixel (exact-2x UpCat layers
                                     with bwd_math FP32, no waux needed)                         */
};

/* One source tensor pair (data, confidence), physical shape (B, C, H, W). */
typedef struct nconv_src {
    const float* x;
    const float* c; /* may be NULL for NCONV_LOAD_THRESH */
    int C, H, W;
} nconv_src;

/* One NConv2d application (models/step1.py:97-149) plus its fused input glue. */
typedef struct nconv_layer {
    int B;
    int Cin, H, W;     /* logical layer input, after the glue (e.g. H = a.H/2 for POOL2)      */
    int Cout, Ho, Wo;  /* output: Ho = (H + 2PH - DH(KH-1) - 1)/SH + 1                         */
    int KH, KW, SH, SW, PH, PW, DH, DW, groups;
    float eps;         /* NConv2d.eps = 1e-7 (step1.py:103)                                     */
    int load_mode;     /* enum nconv_load_mode                                                  */
    float thresh;      /* NCONV_LOAD_THRESH threshold, 0.01 in DNET (step1.py:53)               */
    nconv_src a;       /* plain / thresholded / pooled / skip source                             */
    nconv_src b;       /* low-resolution source of the UPCAT modes (unused otherwise)            */
    const float* weight; /* (Cout, Cin/groups, KH, KW), positive in practice                   */
    const float* bias;   /* (Cout)                                                              */
    const float* wsum;   /* (Cout): s[o] = sum of weight[o] (step1.py:141-144), see nconv_weight_prep */
    int math;            /* enum nconv_math of the forward sums (0 = NCONV_MATH_FP32; unknown: -EINVAL) */
    int bwd_math;        /* enum nconv_math of the backward's products (nconv_bwd, weight and input
                            gradient of the 3x3 / 5x5 layers with Cin > 1): 0 = NCONV_MATH_FP32
                            (exact products), BF16X3 / BF16X9 = split-bf16 matrix cores; unknown:
                            -EINVAL */
    const float* waux;   /* optional precomputed auxiliary weights (NULL = unused):
                            - UPCAT layer: its phase weights (nconv_phase_weights). With exact-fp32
                              math, 16 -> 8 channels (8 + 8), 3x3, stride 1 and an exact nearest 2x
                              upsampling (H = 2 b.H, W = 2 b.W) the forward then convolves source b
                              at its own resolution: 4 fp32 taps of summed weights instead of 9 per
                              pixel (the regrouping (w1 + w2) * v of w1 * v + w2 * v); ignored
                              otherwise;
                            - nconv2 of nconv_fwd_head with exact-fp32 math: the composed
                              confidence weights (nconv_head_weights), required there */
} nconv_layer;

/* ABI version, for the Python loader's sanity check. */
int nconv_abi_version(void);

/* Description of the last error on this thread ("" if none). */
const char* nconv_last_error(void);

/* EnforcePos + confidence-normaliser prologue for n layers in ONE launch.
 * Replaces EnforcePos.__call__ (models/step1.py:190-193, softplus beta=10 threshold=20 at :206-207,
 * applied in place when apply_softplus[i] != 0, i.e. module.training) and the per-layer
 * s = weight.view(Cout,-1).sum(-1) of NConv2d.forward (models/step1.py:141-144).
 * weights[i] has counts[i] = Cout_i * fan_in_i floats; wsums[i] receives Cout_i floats. */
int nconv_weight_prep(int n, float* const* weights, const int* couts, const int* fan_ins,
                      const int* apply_softplus, float* const* wsums, void* stream);

/* Phase weights (nconv_layer.waux) of n UPCAT layers with 8 output channels, 3x3 kernels and 8
 * nearest-2x-upsampled input channels, one launch; call after nconv_weight_prep (they are sums of
 * the current weights: 1, 2 or 4 fp32 weights each, in a fixed order). weights[i] is the layer's
 * (8, cins[i], 3, 3) weight, its upsampled channels are [up_first[i], up_first[i] + 8) (8 for
 * cat(skip, up(low)), 0 for cat(up(low), skip)); wphases[i] receives 1024 floats
 * (= nconv_phase_weights_floats of the layer). The nearest-2x upsampling maps a 3x3 window onto a
 * 2x2 block of source-b pixels; which taps share a pixel depends only on the parity of the window's
 * first row / column (models/step1.py:78-90 glue + :119-122). */
size_t nconv_phase_weights_floats(const nconv_layer* L); /* 0 if L has no phase form */
int nconv_phase_weights(int n, const float* const* weights, const int* cins, const int* up_first,
                        float* const* wphases, void* stream);

/* The inference (eval-mode) weight prologue in ONE launch: the normalisers wsums[i] of n layers
 * (nconv_weight_prep with apply_softplus all 0: EnforcePos is inactive outside training), the exact
 * fused head's auxiliary weights (nconv_head_weights of nconv1 head_w1 (8, 1, 5, 5) and nconv2
 * head_w2 (8, 8, 5, 5) into w21; nconv1's s1 recomputed in-kernel with nconv_weight_prep's
 * arithmetic; skipped when w21 is NULL) and the phase weights of nphase UpCat layers
 * (nconv_phase_weights' arguments). Every output is bitwise what the three separate calls write;
 * the roles read the weights only, so they need no order (replaces three launches per forward). */
int nconv_weight_prologue(int n, float* const* weights, const int* couts, const int* fan_ins,
                          float* const* wsums, const float* head_w1, const float* head_w2, float* w21,
                          int nphase, const float* const* phase_weights, const int* phase_cins,
                          const int* phase_up_first, float* const* wphases, void* stream);

/* The training pass's weight prologue in one launch (replaces models/step1.py:190-207's EnforcePos
 * pre-hooks of DNET's nine layers, whose forward then needs the normalisers and the auxiliaries
 * below: five launches -- nconv_weight_prep, nconv_head_weights, nconv_phase_weights and the three
 * backward box-weight builds -- become one). Layer i (weights[i], couts[i] x fan_ins[i]) gets
 * EnforcePos's softplus in place when softplus[i] (softplus may be NULL: none) and its normalisers
 * in wsums[i]. With w21 != NULL, layers head1 / head2 are nconv1 (8 x 1 x 5 x 5) and nconv2 (8 x 8 x
 * 5 x 5) and w21 receives the exact head's weights (nconv_head_weights, NCONV_HEAD_WEIGHTS_FLOATS);
 * `sync` is then a device counter that is 0 before the call and is left 0 by it (the head's
 * workgroups write nconv1 / nconv2 back once all of them have staged them: one counter per stream
 * that runs this concurrently).
 * Phase layer k is layer phase_layers[k] (8 x 16 x 3 x 3, upsampled channels from phase_up_first[k]
 * = 0 or 8): wphases[k] receives its phase weights (nconv_phase_weights) and, when wboxes and
 * wboxes[k] are non-NULL, wboxes[k] its 1,024 box weights for the phase-form input gradient
 * (nconv_bwd_io.box_weights). Each output is bitwise what the separate calls write after
 * nconv_weight_prep. Every role applies the softplus while staging; a layer is written back by its
 * only reader, or by the last head workgroup. Returns 0 or -EINVAL. */
int nconv_train_prologue(int n, float* const* weights, const int* couts, const int* fan_ins, const int* softplus,
                         float* const* wsums, int head1, int head2, float* w21, unsigned int* sync, int nphase,
                         const int* phase_layers, const int* phase_up_first, float* const* wphases,
                         float* const* wboxes, void* stream);

/* Forward of one NConv2d with fused input glue.
 * Replaces models/step1.py:119-147 (2x F.conv2d, mul, div, bias add, confidence normalisation)
 * plus the glue op that feeds it (step1.py:53 / 62-75 / 78-90).
 * y, cout: (B, Cout, Ho, Wo). */
int nconv_fwd(const nconv_layer* L, float* y, float* cout, void* stream);

/* nconv_fwd plus, in the same launch, the 2x2/s2 max-pool of both outputs (torch semantics:
 * first maximum wins, NaN propagates) into y_pool, cout_pool (B, Cout, Ho/2, Wo/2): the input of
 * the next down layer (models/step1.py:62-75), which then loads it with NCONV_LOAD_PLAIN instead
 * of re-reading and pooling the full-resolution tensors. Built for the tiled DNET layer shapes
 * (returns -EOPNOTSUPP otherwise). argmax (may be NULL; exact-fp32 tiled layers only): one 32-bit
 * word per pooled element (not a byte: the backward's staging then loads it like its float
 * operands, with no conversion ahead of its use), the window slot (2*row + column) of y's first
 * maximum in bits 0-1 and of cout's in bits 2-3 -- what nconv_bwd_ex routes the pooled tensors' gradient by (the indices of
 * max_pool2d_with_indices, step1.py:62-75 under autograd). */
int nconv_fwd_pooled(const nconv_layer* L, float* y, float* cout, float* y_pool, float* cout_pool,
                     unsigned int* argmax, void* stream);

/* Fused head: nconv1 on the thresholded sparse depth (models/step1.py:53-57;
 * L1: Cin 1, Cout 8, 5x5, padding 2, NCONV_LOAD_THRESH) is evaluated while staging nconv2's input
 * tile (step1.py:58; L2: 8 -> 8, 5x5, padding 2, stride 1; its sources are not read), so nconv1's
 * 8-channel output never reaches HBM. Writes nconv2's y, cout (B, 8, H, W) and their 2x2 max-pooled
 * copies (B, 8, H/2, W/2) like nconv_fwd_pooled. L2->math selects the arithmetic:
 *  - NCONV_MATH_FP32: exact fp32 (nconv_fwd_head.hip). nconv1 visits only the nonzero taps of each
 *    window (bitwise its dense sums); nconv2's confidence mass D2 is the 9x9 convolution of the
 *    binary mask c0 with the composed weights sum_i W2[o,i] (x) W1[i] / s1[i] that L2->waux must
 *    hold (nconv_head_weights), on the bf16 matrix cores with exact products (c0 is 0 or 1, each
 *    weight the exact sum of three bf16 parts) and fp32 accumulation, except in tiles whose window
 *    nconv2's zero padding truncates;
 *  - NCONV_MATH_BF16X3 / BF16X9: the matrix-core head (nconv1 uses the same split).
 * Training (exact fp32 only; all three or NULL): y1, cout1 (B, 8, H, W) receive nconv1's outputs
 * (bitwise nconv_fwd's: the nonzero-tap sums are the dense sums) for the backward, argmax the
 * pooling codes as nconv_fwd_pooled's. */
int nconv_fwd_head(const nconv_layer* L1, const nconv_layer* L2, float* y, float* cout, float* y_pool,
                   float* cout_pool, unsigned int* argmax, float* y1, float* cout1, void* stream);

/* Auxiliary weights of the exact fused head (L2->waux of nconv_fwd_head): w21 receives
 * NCONV_HEAD_WEIGHTS_FLOATS floats. First the composed confidence weights W21[o][qh][qw] = sum_i
 * (1 / s1[i]) sum W2[o][i][kh][kw] W1[i][kh'][kw'] over kh + kh' = qh, kw + kw' = qw (fp64, rounded
 * once to fp32; s1 = L1->wsum), each split exactly into three bf16 parts and laid out as the A
 * operands of the head's matrix-core D2 (1536 dwords, nconv_fwd_head.hip kFrag), then nconv2's
 * weights transposed to [i][kh][kw][o] (1600 floats). nconv1's cout = D1 / s1
 * (models/step1.py:141-147), so nconv2's D2 = sum_i W2[o,i] * c1[i] = W21[o] * c0 wherever nconv2's
 * window is not truncated by its zero padding. Call after nconv_weight_prep. */
#define NCONV_HEAD_WEIGHTS_FLOATS 3136
int nconv_head_weights(const nconv_layer* L1, const nconv_layer* L2, float* w21, void* stream);

/* Fused tail: the last 3x3 NConv (nconv6, step1.py:88-90) with its 1x1 successor (nconv7,
 * step1.py:92) evaluated in the epilogue, written straight into the (cropped) output
 * (step1.py:94). L6 describes nconv6 (stride 1, no dilation, groups 1). Output pixel (r, c) of
 * `out` (B, 1, out_h, out_w) is nconv7's output at (r + crop0, c + crop0) of its (Ho6+2*p7) x
 * (Wo6+2*p7) grid, i.e. nconv6 pixel (r + crop0 - p7, c + crop0 - p7); positions in nconv7's zero
 * border get b7. crop0 = 1 is DNET's crop; crop0 = 0 with the full grid is nconv7's whole output.
 * out_c (nullable) receives the matching output confidence. Training (exact fp32, exactly-2x
 * phase form only; both or NULL): y6, cout6 (B, Cout6, Ho6, Wo6) receive nconv6's outputs, which
 * the backward reads; the output window must then cover every nconv6 pixel (crop0 <= p7,
 * crop0 + out_h - p7 >= Ho6, crop0 + out_w - p7 >= Wo6), else -EINVAL. */
int nconv_fwd_tail(const nconv_layer* L6, const float* w7, const float* b7, const float* wsum7,
                   int cin7, int p7, float eps7, float* out, float* out_c, int out_h, int out_w, int crop0,
                   float* y6, float* cout6, void* stream);

/* Which kernels nconv_fwd (without fused pooling) and nconv_bwd run for L (enum nconv_kernel):
 * the arithmetic a descriptor selects, made observable to hosts and tests. Host-only (no device
 * work); any output pointer may be NULL. Returns 0 or -EINVAL for an invalid descriptor. */
int nconv_plan(const nconv_layer* L, int* fwd_kernel, int* dgrad_kernel, int* wgrad_kernel);

/* Workspace needed by nconv_bwd (bytes). */
size_t nconv_bwd_workspace_bytes(const nconv_layer* L);

/* Backward of nconv_fwd (autograd of models/step1.py:116-149 plus the glue's backward:
 * max_pool2d routes to the first maximum of each window, nearest-upsample sums, cat splits).
 * Inputs: y, cout (the forward outputs), gy, gcout (their gradients; gcout may be NULL = 0).
 * Outputs (any may be NULL if not needed):
 *   gxa, gca : gradients of source a's (x, c)      — same shape as a
 *   gxb, gcb : gradients of source b's (x, c)      — same shape as b (UPCAT modes)
 *              with (flags & NCONV_BWD_ACCUMULATE) these four are added into; otherwise every
 *              element is overwritten (no zero-fill needed)
 *   gw       : (Cout, Cin/groups, KH, KW) weight gradient, OVERWRITTEN
 *   gbias    : (Cout) bias gradient, OVERWRITTEN
 * The closed form: gN = gy/(D+eps), gD = -gy*N/(D+eps)^2 + gcout/s,
 *   gb = sum gy, gs = -sum gcout*D/s^2, gW = corr(x*c, gN) + corr(c, gD) + gs,
 *   g(xc) = W^T * gN, gx = g(xc)*c, gc = W^T * gD + g(xc)*x.
 * D and N/(D+eps) are recovered from the saved outputs as cout*s and y-b. */
#define NCONV_BWD_ACCUMULATE 1u
/* (flags & NCONV_BWD_DEFER_REDUCE): the weight gradient is left in the workspace as per-workgroup
 * partial rows and nconv_bwd returns their number (>= 0; 0 when gw and gbias are both NULL) instead
 * of 0; gw / gbias are written by a later nconv_wgrad_reduce over that workspace (which must stay
 * untouched until then). A training backward defers every layer and reduces them all in two
 * launches instead of two per layer. Same sums, same fixed order: the result is bitwise that of
 * the undeferred call. */
#define NCONV_BWD_DEFER_REDUCE 2u
/* Accepted and ignored since ABI 21: the input and the weight gradient always run as two kernels
 * (the one-kernel form of ABI 19-20 measured slower and was removed). */
#define NCONV_BWD_SEPARATE 4u

int nconv_bwd(const nconv_layer* L, const float* y, const float* cout, const float* gy,
              const float* gcout, float* gxa, float* gca, float* gxb, float* gcb, float* gw,
              float* gbias, void* workspace, size_t workspace_bytes, unsigned flags, void* stream);

/* nconv_bwd with its tensors in one struct, plus the gradient arriving through a 2x2 max-pool of
 * this layer's outputs (training: the next down layer read the y_pool / cout_pool that
 * nconv_fwd_pooled materialised, so its input gradient is pooled-sized): gy_pool, gcout_pool
 * (B, Cout, Ho/2, Wo/2) are added to gy / gcout at each window's first maximum, as pool_argmax
 * (that nconv_fwd_pooled call's codes) records -- the max_pool2d backward of step1.py:62-75 summed
 * with the other consumer's gradient, without a full-resolution read-modify-write. All three or
 * none; with them, built for the exact-fp32 8->8 5x5 stride-1 layers with NCONV_LOAD_PLAIN
 * (-EOPNOTSUPP otherwise). Returns as nconv_bwd. */
typedef struct nconv_bwd_io {
    const float* y;
    const float* cout;
    const float* gy;
    const float* gcout;             /* may be NULL (= 0) */
    float* gxa;
    float* gca;
    float* gxb;
    float* gcb;
    float* gw;
    float* gbias;
    const float* gy_pool;           /* optional pooled-output gradient (see above) */
    const float* gcout_pool;
    const unsigned int* pool_argmax;
    /* optional: the weight gradient of the layer that produced L's input, fused into L's input
     * gradient (DNET training: nconv2's backward computes nconv1's gW / gb in-tile, so nconv1's
     * input gradient never reaches HBM and nconv1 needs no nconv_bwd). head = nconv1's descriptor
     * (1 -> 8, 5x5, padding 2, stride 1, NCONV_LOAD_THRESH on the sparse depth; its output is L's
     * source a); L must be an exact-fp32 8 -> 8 5x5 layer with NCONV_LOAD_PLAIN. head_workspace:
     * nconv_bwd_head_workspace_bytes(L) bytes. Without NCONV_BWD_DEFER_REDUCE head_gw / head_gbias
     * are written in this call; with it head_nparts receives the partial-row count for
     * nconv_wgrad_reduce (layer head, workspace head_workspace). gxa / gca (nconv1's output
     * gradient) are then optional. */
    const nconv_layer* head;
    void* head_workspace;
    size_t head_workspace_bytes;
    float* head_gw;
    float* head_gbias;
    int head_nparts;                /* out */
    /* optional: the backward of the 1x1 layer that consumes L's outputs, fused into L's (DNET
     * training: nconv7, 8 -> 1, 1x1, padding 2, after nconv6). tail = nconv7's descriptor; tail_y,
     * tail_cout, tail_gy its outputs and their gradient, (B, 1, Ho + 4, Wo + 4); its cout gradient
     * is taken as 0 by nconv_bwd_ex (DNET without a confidence loss discards nconv7's confidence) and
     * is the extra plane of nconv_bwd_tail_conf below. L's gy / gcout are then formed in-kernel
     * from them (gy, gcout above are ignored and may be NULL), so nconv7's input gradient never
     * reaches HBM; nconv7's weight gradient goes to tail_gw (tail_workspace of
     * nconv_bwd_tail_workspace_bytes(L) bytes; with NCONV_BWD_DEFER_REDUCE tail_nparts partial rows
     * for nconv_wgrad_reduce, layer tail). nconv7's bias gradient (the sum of tail_gy) is left to
     * the caller (it is computed by the call that requests L's gw / gbias: a call with only the
     * input gradients computes none of nconv7's; tail_gw without gw / gbias is -EINVAL). L must
     * be nconv6's exact-fp32 geometry (16 -> 8 3x3, padding 0, upsample-first exactly-2x concat). */
    const nconv_layer* tail;
    const float* tail_y;
    const float* tail_cout;
    const float* tail_gy;
    void* tail_workspace;
    size_t tail_workspace_bytes;
    float* tail_gw;
    int tail_nparts;                /* out */
    /* ABI 20. optional: the box weights of an exactly-2x UPCAT layer's phase-form input gradient
     * (nconv_train_prologue wboxes), else built by a launch of this call. */
    const float* box_weights;
    /* ABI 20. The tail planes' extent: all zero = nconv7's whole (Ho + 4) x (Wo + 4) grid;
     * otherwise (B, 1, tail_h, tail_w) holding the grid from row / column tail_crop0 (DNET's crop,
     * step1.py:94: the training output written cropped by nconv_fwd_tail); gradient outside the
     * window is 0. */
    int tail_crop0;
    int tail_h;
    int tail_w;
} nconv_bwd_io;

int nconv_bwd_ex(const nconv_layer* L, nconv_bwd_io* io, void* workspace, size_t workspace_bytes,
                 unsigned flags, void* stream);
size_t nconv_bwd_head_workspace_bytes(const nconv_layer* L);
size_t nconv_bwd_tail_workspace_bytes(const nconv_layer* L);
/* nconv_bwd_ex with the fused tail's cout gradient (a new entry point: nconv_bwd_io is unchanged, so
 * NCONV_ABI_VERSION stays 27). tail_gcout: the gradient of io->tail_cout, the same extent and crop
 * window as io->tail_gy (0 outside the window); NULL: exactly nconv_bwd_ex. With it nconv7's
 * {gN, gD} take gcout as the general layer backward does (gD += gcout / s), and nconv7's weight
 * gradient gains its normaliser term -(sum gcout * cout) / s, summed over nconv7's grid in a fixed
 * order. -EINVAL where tail_gcout is given without io->tail; -EOPNOTSUPP where L is not the fused
 * tail's exact-fp32 geometry (as nconv_bwd_ex with io->tail). */
int nconv_bwd_tail_conf(const nconv_layer* L, nconv_bwd_io* io, const float* tail_gcout, void* workspace,
                        size_t workspace_bytes, unsigned flags, void* stream);

/* Weight / bias gradients of n (1..16) layers whose nconv_bwd ran with NCONV_BWD_DEFER_REDUCE:
 * layers[k] the descriptor of that call (its weight normaliser wsum is read), workspaces[k] and
 * nparts[k] its workspace and return value, gw[k] / gbias[k] the outputs (either may be NULL;
 * layers with nparts[k] == 0 are skipped). Two launches on `stream`. Returns 0 or -EINVAL. */
int nconv_wgrad_reduce(int n, const nconv_layer* layers, void* const* workspaces, const int* nparts,
                       float* const* gw, float* const* gbias, void* stream);

/* nconv_wgrad_reduce plus nsum plain sums in the same two launches (n + nsum in 1..16): sum_out[k]
 * = the sum of sum_x[k][0 .. sum_n[k]) in a fixed order (bitwise deterministic; DNET training:
 * nconv7's bias gradient, the sum of its output gradient, without two launches of its own).
 * sum_workspace: nconv_sum_workspace_bytes(nsum) bytes. n may be 0. Returns 0 or -EINVAL. */
int nconv_wgrad_reduce_ex(int n, const nconv_layer* layers, void* const* workspaces, const int* nparts,
                          float* const* gw, float* const* gbias, int nsum, const float* const* sum_x,
                          const long long* sum_n, float* const* sum_out, void* sum_workspace,
                          size_t sum_workspace_bytes, void* stream);
size_t nconv_sum_workspace_bytes(int nsum);

/* ------------------------------------------------------------------------------------------
 * Dense convolutions of the RGB-guided model on the matrix cores (fp32 MFMA, exact f32 products).
 * Replace the nn.Conv2d / nn.ConvTranspose2d (+ eval BatchNorm + ReLU + residual add + torch.cat)
 * sequences of models/step2.py: RGBEncoder (:134-154), ConvBlock (:290-297), Basic2d (:178-195),
 * Basic2dTrans (:197-214), UpCat / NewFusionBlock cat (:173-175, :229-231), Conv3x3 heads (:156-158,
 * :259, :278). Inference (eval) semantics: BatchNorm uses its running statistics, folded into
 * the packed weights (scale) and the bias.
 * ------------------------------------------------------------------------------------------ */
enum nconv_dense_kind {
    NCONV_DENSE_3X3 = 0,            /* Conv2d 3x3, padding 1, stride 1 or 2                      */
    NCONV_DENSE_1X1 = 1,            /* Conv2d 1x1, padding 0, stride 1 or 2                      */
    NCONV_DENSE_TRANSPOSED_4X4 = 2, /* ConvTranspose2d 4x4, stride 2, padding 1 (Ho = 2H, or the
                                       cropped 2H - 1)                                           */
    NCONV_DENSE_CONV4X4_S2 = 3      /* Conv2d 4x4, stride 2, padding 1, Ho = (H - 1) / 2 + 1: the
                                       input gradient of the transposed convolution              */
};

typedef struct nconv_dense_conv {
    int B;
    const float* x0; int C0;   /* input = cat(x0, x1) along channels: x0 (B, C0, H, W)          */
    const float* x1; int C1;   /* x1 (B, C1, H, W), or NULL / 0                                   */
    int H, W;
    int Cout, Ho, Wo;          /* any Cout >= 1 (tiled by 32 or 64 output channels)               */
    int kind, stride;
    const float* wpack;        /* nconv_dense_pack output                                         */
    const float* bias;         /* (Cout) or NULL                                                   */
    int relu;                  /* 1: max(., 0) after the bias                                      */
    const float* wshort;       /* optional packed 1x1 shortcut (same stride) added after the ReLU  */
    float* out;                /* output channels [out_c0, out_c0 + Cout) of (B, out_C, Ho, Wo)    */
    int out_C, out_c0;
    int math;                  /* enum nconv_dense_math (ABI 22; 0 = fp32 MFMA)                     */
} nconv_dense_conv;

/* Arithmetic of every kind but the 1x1 (3x3 stride 1 or 2 with or without the 1x1 shortcut, the
 * transposed 4x4, the 4x4 stride 2: the RGB encoder, the fusion decoder and their input
 * gradients); the 1x1 always runs NCONV_DENSE_MATH_FP32.
 * Both split forms sum in fp32 on the matrix cores in another order than the fp32-MFMA kernel (an
 * fmaf chain), so results agree with it to fp32 accumulation error, not bitwise. */
enum nconv_dense_math {
    NCONV_DENSE_MATH_FP32 = 0,  /* v_mfma_f32_32x32x2_f32: exact f32 products                      */
    NCONV_DENSE_MATH_BF16X9 = 2,/* exact products on the bf16 matrix cores: both operands split into
                                   three bf16 parts (an exact decomposition), all nine partial
                                   products (each exact in fp32) accumulated in fp32              */
    NCONV_DENSE_MATH_BF16X6 = 3 /* the six largest of those nine terms: each product within
                                   ~2^-23 relative (the dropped v1*w2 + v2*w1 + v2*w2)             */
};

/* Floats of a packed weight buffer for (kind, Cin, Cout) (the fp32 image, then the pre-split bf16
 * image of the split-bf16 maths, ABI 22). */
size_t nconv_dense_packed_floats(int kind, int Cin, int Cout);

/* Pack w — Conv2d (Cout, Cin, k, k) or ConvTranspose2d (Cin, Cout, 4, 4) — into the kernel's
 * layout, multiplying output channel o by scale[o] if scale != NULL (eval BatchNorm folding).
 * The layout depends on (kind, Cin, Cout) only: a pack is valid for every call with those. */
int nconv_dense_pack(int kind, int Cin, int Cout, const float* w, const float* scale, float* wpack,
                     void* stream);

/* out[:, out_c0:out_c0+Cout] = [relu](conv(cat(x0, x1)) + bias) [+ conv1x1_shortcut(cat(x0, x1))] */
int nconv_dense_conv_fwd(const nconv_dense_conv* c, void* stream);

/* 3x3 (padding 1, stride 1) convolution to one output channel plus a residual:
 * out = conv3x3(x; w (1, Cin, 3, 3)) + res, all (B, ., H, W); res may be NULL
 * (the depth heads `depth + Conv3x3(fout)`, models/step2.py:259,278). */
int nconv_conv3x3_c1(const float* x, int B, int Cin, int H, int W, const float* w, const float* res,
                     float* out, void* stream);

/* Bilinear resampling with align_corners=True of (B, C, H, W) planes to (B, C, Ho, Wo): the guided
 * model's depth downsampling F.interpolate(depth, scale_factor=1/k, mode="bilinear",
 * align_corners=True) (models/step2.py:249,277), with the sampling arithmetic of the reference's
 * CPU kernel: scale = fp32(H-1) / (Ho-1), source coordinate fp32(scale * o), truncated index,
 * fp32 lambdas, blend fma(l0h, fma(l0w, a00, l1w*a01), l1h*fma(l0w, a10, l1w*a11)). x and y must
 * not overlap. */
int nconv_bilinear_ac(const float* x, int B, int C, int H, int W, float* y, int Ho, int Wo, void* stream);

/* ------------------------------------------------------------------------------------------
 * Training of the guided model: the weight gradient of a dense convolution.
 * Replaces the autograd of nn.Conv2d / nn.ConvTranspose2d (convolution_backward, weight part) for
 * the layers of models/step2.py listed above. The input gradient of a convolution is another
 * convolution of dL/dy and runs on nconv_dense_conv_fwd with re-arranged weights (3x3 / 1x1
 * stride 1: transposed, flipped; stride 2: NCONV_DENSE_TRANSPOSED_4X4 with the 3x3 / 1x1 kernel
 * embedded, output cropped to H x W; transposed 4x4: NCONV_DENSE_CONV4X4_S2, same weights).
 * The bias gradient is the sum of dL/dy over images and pixels.
 * ------------------------------------------------------------------------------------------ */
typedef struct nconv_dense_wgrad {
    int B;
    int kind, stride;          /* the forward convolution: NCONV_DENSE_3X3 / _1X1 (stride 1|2),
                                  NCONV_DENSE_TRANSPOSED_4X4 (stride 2)                           */
    const float* x0; int C0;   /* forward input = cat(x0, x1) along channels, (B, C0 + C1, H, W)  */
    const float* x1; int C1;   /* NULL / 0 for one source                                         */
    int H, W;
    const float* gy;           /* dL/dy, (B, Cout, Ho, Wo)                                        */
    int Cout, Ho, Wo;
    float* gw;                 /* OVERWRITTEN: Conv2d (Cout, Cin, k, k) / ConvTranspose2d
                                  (Cin, Cout, 4, 4). Limits: Cout <= 96 (conv), Cin <= 96
                                  (transposed), Cin <= 64 (1x1)                                   */
    int math;                  /* enum nconv_dense_math (ABI 22): the split-bf16 maths run the 3x3
                                  gradient (stride 1 or 2, >= 4 input channels) on the bf16 matrix
                                  cores; every other shape the fp32 MFMA kernel                   */
} nconv_dense_wgrad;

/* Workspace of nconv_dense_conv_wgrad in bytes (0 if the descriptor is invalid). */
size_t nconv_dense_wgrad_workspace_bytes(const nconv_dense_wgrad* g);

/* gw = dL/dW: deterministic (fixed-order reduction of per-workgroup partial sums). */
int nconv_dense_conv_wgrad(const nconv_dense_wgrad* g, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Training-mode BatchNorm2d + optional ReLU: batch statistics, running statistics updated in
 * place (momentum, unbiased running variance) — the nn.BatchNorm2d(train) -> nn.ReLU pairs of
 * models/step2.py:139-143 (RGBEncoder), :189-191 (Basic2d), :207-213 (Basic2dTrans) — and its
 * backward (the ReLU mask recomputed from x). Deterministic (fixed-order reductions).
 * ------------------------------------------------------------------------------------------ */
typedef struct nconv_bn_train {
    int B, C, H, W;
    const float* x;            /* (B, C, H, W) input                                              */
    const float* gamma;        /* (C) or NULL (= 1)                                               */
    const float* beta;         /* (C) or NULL (= 0)                                               */
    float* running_mean;       /* (C) updated by the forward, or NULL                             */
    float* running_var;        /* (C) updated by the forward (unbiased variance), or NULL         */
    float momentum, eps;
    int relu;                  /* 1: y = max(BN(x), 0)                                            */
    float* y;                  /* (B, C, H, W) forward output                                     */
    float* mean;               /* (2 C) batch mean as two fp32 words, [c] + [C + c] (ABI 23: one
                                  word is half an ulp of the mean off, which a channel of large
                                  mean and small spread sees times invstd in every output):
                                  written by the forward, read by the backward                    */
    float* invstd;             /* (C) 1/sqrt(biased batch variance + eps): likewise               */
} nconv_bn_train;

/* Workspace of nconv_bn_train_fwd / _bwd in bytes (0 if the descriptor is invalid). */
size_t nconv_bn_workspace_bytes(const nconv_bn_train* p);

int nconv_bn_train_fwd(const nconv_bn_train* p, void* workspace, size_t workspace_bytes, void* stream);

/* gx = dL/dx (NULL: skip), ggamma / gbeta = dL/dgamma, dL/dbeta (OVERWRITTEN; NULL: skip),
 * from gy = dL/dy and the forward's x, mean, invstd. */
int nconv_bn_train_bwd(const nconv_bn_train* p, const float* gy, float* gx, float* ggamma, float* gbeta,
                       void* workspace, size_t workspace_bytes, void* stream);

/* Backward of the ReLU after a biased convolution and its bias gradient (ConvBlock, step2.py:
 * 290-297, bias + ReLU fused in nconv_dense_conv_fwd): g_masked = g * (out > 0) (out = the
 * forward's ReLU output; out == NULL: no ReLU, g_masked unused), gbias[c] = sum over images and
 * pixels of the masked gradient (NULL: skip). All (B, C, H, W) except gbias (C). */
size_t nconv_relu_bias_bwd_workspace_bytes(int B, int C, int H, int W);
int nconv_relu_bias_bwd(int B, int C, int H, int W, const float* g, const float* out, float* g_masked,
                        float* gbias, void* workspace, size_t workspace_bytes, void* stream);

/* Training loss of the reference (utils.py:95-151 calculate_loss) on B (H, W) planes: the training
 * loop calls it on the whole (B, 1, H, W) batch (train_step1.py:63), the validation loop on element
 * [0] (utils.py:36; B = 1). rec = r masked to 0 where t == 0; use_gradient_loss != 0:
 * L = 0.8 sqrt(mean (rec - t)^2) + 0.2 (mean |Sobel_x(t - rec)| + mean |Sobel_y(t - rec)|), else
 * L = mean (rec - t)^2; means over B*H*W, each image's Sobel response zero-padded on its own
 * (F.conv2d, padding 1). r and t are fp32 with image / row strides in elements (r may be a cropped
 * view). nconv_depth_loss_fwd writes L to loss[0] (device) and keeps the backward's coefficients in
 * the workspace, which nconv_depth_loss_bwd reads: g (contiguous B x H x W, OVERWRITTEN) =
 * gloss[0] * dL/dr (gloss NULL: 1). Deterministic (fixed-order reductions). */
size_t nconv_depth_loss_workspace_bytes(int B, int H, int W);
/* -EINVAL "plane too large" where an operand's extent ((H - 1) * row stride + W) * 4 reaches 2^31
 * bytes (a plane is read through 32-bit byte offsets), like the other entry points that take views. */
int nconv_depth_loss_fwd(const float* r, long long r_image_stride, long long r_row_stride, const float* t,
                         long long t_image_stride, long long t_row_stride, int B, int H, int W, int use_gradient_loss,
                         float* loss, void* workspace, size_t workspace_bytes, void* stream);
/* The same checks as the forward, the 2^31-byte extent limit ("plane too large") included. */
int nconv_depth_loss_bwd(const float* r, long long r_image_stride, long long r_row_stride, const float* t,
                         long long t_image_stride, long long t_row_stride, int B, int H, int W, int use_gradient_loss,
                         const float* gloss, const void* workspace, size_t workspace_bytes, float* g, void* stream);

/* Confidence loss (new entry points only: no existing struct or signature changes, so
 * NCONV_ABI_VERSION stays 27). The loss the NConv authors train the output confidence with (Eldesokey,
 * Felsberg, Khan, TPAMI 2019; ConfLossDecay in their code) on B (H, W) planes of the prediction r, the
 * output confidence c and the target t, all fp32 with image / row strides in elements (r and c may be
 * cropped views). The rule, operation by operation in fp32, no contraction:
 *     v    = (t != 0)
 *     d    = r - t
 *     a    = |d|
 *     NCONV_CONF_LOSS_SMOOTH_L1 (beta > 0):
 *         e  = a < beta ? ((0.5f * a) * a) / beta : a - 0.5f * beta
 *         de = a < beta ? d / beta : (d > 0 ? 1 : -1)
 *     NCONV_CONF_LOSS_L2:
 *         e  = d * d
 *         de = 2 * d
 *     term = v ? e - (lam * c) * (1.0f - e) : 0      (the published err - lam (c v - err c v), lam = 1 / p)
 *     L    = (sum term) / n, n = B * H * W: the mean over all pixels, as published
 *     k    = gloss * (1.0f / (float)n)                (gloss NULL: 1)
 *     g_r  = v ? (k * de) * (1.0f + lam * c) : 0
 *     g_c  = v ? -((k * lam) * (1.0f - e)) : 0
 * lam is read from a device fp32 scalar when the kernels run, so a captured training step decays it
 * without another capture. nconv_conf_loss_fwd writes L to loss[0] (device): fp32 partials over fixed
 * 16 x 64 tiles (1024 terms each), tiles and images combined in double in a fixed order, no atomics.
 * nconv_conf_loss_bwd OVERWRITES g_r and g_c (contiguous B x H x W; either may be NULL: skipped); it
 * reads no workspace. The checks are nconv_depth_loss_*'s, the 2^31-byte extent limit ("plane too
 * large") included; also -EINVAL: beta <= 0 or NaN, an err_kind outside the enum, null lam. */
enum nconv_conf_loss_err {
    NCONV_CONF_LOSS_SMOOTH_L1 = 0,
    NCONV_CONF_LOSS_L2 = 1
};
size_t nconv_conf_loss_workspace_bytes(int B, int H, int W);
int nconv_conf_loss_fwd(const float* r, long long r_image_stride, long long r_row_stride, const float* c,
                        long long c_image_stride, long long c_row_stride, const float* t, long long t_image_stride,
                        long long t_row_stride, int B, int H, int W, int err_kind, float beta, const float* lam,
                        float* loss, void* workspace, size_t workspace_bytes, void* stream);
int nconv_conf_loss_bwd(const float* r, long long r_image_stride, long long r_row_stride, const float* c,
                        long long c_image_stride, long long c_row_stride, const float* t, long long t_image_stride,
                        long long t_row_stride, int B, int H, int W, int err_kind, float beta, const float* lam,
                        const float* gloss, float* g_r, float* g_c, void* stream);

/* Depth-completion evaluation figures on B (H, W) planes, as twelve raw sums per image. The
 * reference reports only its validation loss (utils.py:18-40); the KITTI (MAE, RMSE, iMAE, iRMSE)
 * and NYU (REL, squared REL, RMSE(log), delta < 1.25^k) figures a user compares with published
 * numbers are ~40 PyTorch elementwise / reduction launches per frame and one .item() per figure.
 * This replaces them with two launches and no host synchronisation. pred and gt are fp32 with
 * image / row strides in elements (pred may be a cropped view whose first element is not 16-byte
 * aligned). A bound of 0 is absent. A pixel is valid iff gt > 0, gt >= gt_min and gt <= gt_max;
 * p = pred clamped into [clamp_lo, clamp_hi], g = gt, e = p - g; a valid pixel is positive iff
 * p > 0 (a NaN prediction at a valid pixel is not positive and makes sums 2-5 NaN). Per image:
 *    0  n_valid                  4  sum |e| / g               8  sum (ln p - ln g)^2
 *    1  n_pos                    5  sum e^2 / g               9  #{max(p/g, g/p) < 1.25}
 *    2  sum |e|                  6  sum |1/p - 1/g|          10  #{max(p/g, g/p) < 1.5625}
 *    3  sum e^2                  7  sum (1/p - 1/g)^2        11  #{max(p/g, g/p) < 1.953125}
 * sums 2-5 over the valid pixels, 6-11 over the positive ones. sums (B x 12 doubles, OVERWRITTEN;
 * NULL: skip) receives each image's row; accum (12 doubles; NULL: skip) is then increased by the
 * rows of images 0 .. B-1 in that order (a running total over calls). Per-pixel terms in fp32 (IEEE
 * division, logf), fp32 partials of 16 x 64 pixel tiles, tiles and images combined in double in a
 * fixed order: deterministic (no atomics), counts exact. workspace must be 8-byte aligned. */
#define NCONV_DEPTH_METRICS_SUMS 12
size_t nconv_depth_metrics_workspace_bytes(int B, int H, int W);
int nconv_depth_metrics(const float* pred, long long p_image_stride, long long p_row_stride, const float* gt,
                        long long g_image_stride, long long g_row_stride, int B, int H, int W, float gt_min,
                        float gt_max, float clamp_lo, float clamp_hi, double* sums, double* accum, void* workspace,
                        size_t workspace_bytes, void* stream);

/* Raw sensor frames -> the network's fp32 tensors, in one launch per batch (the reference decodes on
 * the host: torch.FloatTensor(cv2.imread(..)).permute(2, 0, 1) and imread(..) / 256.0,
 * dataset/kittiloader.py:62-79, and ships fp32 across the link: 20 bytes per pixel for rgb + depth +
 * gt against 7 as stored). Every source is a strided view given by its base pointer, image stride
 * and row stride in BYTES, so a crop is a pointer offset plus strides.
 *   rgb    uint8, interleaved 3-channel (B, h, w, 3); any byte alignment, row stride >= 3 w
 *          -> rgb_out fp32 (B, 3, h, w) contiguous, exactly float(byte); reverse != 0 writes the
 *          channels in reverse order (RGB source -> BGR planes, cv2.imread's order). NULL: no RGB.
 *   plane  up to two single-channel (B, h, w) planes (sparse depth, ground truth), each with its
 *          own dtype, right shift (integers only, 0..15) and fp32 scale
 *          -> out fp32 (B, 1, h, w) contiguous = float(v >> shift) * scale; F32: v * scale (one
 *          fp32 multiply). A 16-bit KITTI PNG in metres: U16, shift 0, scale 1/256; as the
 *          reference's 8-bit imread sees it: U16, shift 8, scale 1/256. src NULL: absent.
 *          U16 / F32 sources must be aligned to their element (base and strides).
 * No byte outside a view's extent [base, base + (B-1) image_stride + (h-1) row_stride + w * element)
 * is read. Wide loads where base and strides are 4-byte aligned (F32: 16-byte), element-wide
 * range-checked loads otherwise. One kernel, no workspace. */
enum nconv_frame_dtype { NCONV_FRAME_U8 = 0, NCONV_FRAME_U16 = 1, NCONV_FRAME_F32 = 2 };

typedef struct nconv_frame_plane {
    const void* src;        /* NULL: absent                                                  */
    long long image_stride; /* bytes (ignored when B == 1)                                   */
    long long row_stride;   /* bytes, >= w * element size                                    */
    int dtype;              /* enum nconv_frame_dtype                                        */
    int shift;              /* 0..15; 0 for F32                                              */
    float scale;
    float* out;             /* (B, 1, h, w) contiguous fp32                                  */
} nconv_frame_plane;

/* (the struct tag shares its name with the entry point: spell the type `struct nconv_frame_ingest`
 * or nconv_frame_ingest_desc) */
typedef struct nconv_frame_ingest {
    int B, h, w;
    int reverse;                   /* != 0: rgb_out's planes in reverse channel order        */
    const unsigned char* rgb;      /* NULL: no RGB                                           */
    long long rgb_image_stride;    /* bytes (ignored when B == 1)                            */
    long long rgb_row_stride;      /* bytes, >= 3 w                                          */
    float* rgb_out;                /* (B, 3, h, w) contiguous fp32                           */
    nconv_frame_plane plane[2];
} nconv_frame_ingest_desc;

int nconv_frame_ingest(const struct nconv_frame_ingest* d, void* stream);

/* A prediction as 16-bit fixed point (KITTI's submission format is a 16-bit PNG of depth x 256):
 * out[b][i][j] = clamp(round_to_nearest_even(pred * scale), 0, 65535), NaN -> 0, the product one
 * fp32 rounding. pred is fp32 with image / row strides in elements, as nconv_depth_metrics takes it
 * (a cropped view such as DNET's output works); out is uint16 (B, 1, H, W) contiguous, 2-byte
 * aligned. scale must be positive. One kernel, no workspace. */
int nconv_depth_export_u16(const float* pred, long long image_stride, long long row_stride, int B, int H, int W,
                           float scale, unsigned short* out, void* stream);

/* ABI 26. A completed depth map and the camera intrinsics -> a metric 3-D point cloud. The reference
 * has no counterpart: its loaders return the 3x3 intrinsics `k` of every frame, principal point
 * shifted by the crop (this package's data.py:121-122, 246-247; dataset/kittiloader.py), and nothing
 * reads them. With PyTorch ops the same result is a meshgrid, three elementwise passes, a boolean-mask
 * index and a host synchronisation for the point count.
 * Pixel (b, i, j) with z = depth[b][i][j] is valid iff
 *     z > z_min && z <= z_max && (conf == NULL || conf[b][i][j] >= conf_min)
 * (comparisons: a NaN depth or confidence is not valid) and its point is
 *     x = ((float)j - cx) * z / fx,   y = ((float)i - cy) * z / fy,   z
 * each operation one fp32 rounding in that order, the division IEEE. fx, fy, cx, cy = K[0][0],
 * K[1][1], K[0][2], K[1][2] of image b's row-major 3x3 matrix at k + b * k_image_stride, read on the
 * device; the other five entries of K are NOT read (no skew, no distortion). k_image_stride = 0: one
 * camera for the whole batch.
 * depth, conf: fp32 (B, H, W) views, image / row strides in elements (a cropped view such as DNET's
 * output works), 4-byte aligned. color (optional), by color_kind:
 *   NCONV_COLOR_F32_PLANAR      fp32 (B, 3, H, W) view, image / channel / row strides in floats (the
 *                               tensors the models take); a value v becomes clamp(rintf(v), 0, 255),
 *                               NaN -> 0
 *   NCONV_COLOR_U8_INTERLEAVED  uint8 (B, H, W, 3), image / row strides in bytes (the raw=True
 *                               loaders' frames); color_channel_stride is ignored
 * and the point's colour is 3 x uint8 in the source's channel order, reversed when reverse != 0.
 * The zero value of every optional field is "absent / default": conf NULL = no gate, color NULL /
 * NCONV_COLOR_NONE = no colour, conf_min 0, z_min 0, z_max 0 (beside a z_min >= 0, where it would
 * select nothing) = FLT_MAX, so +inf is not valid.
 * No byte outside a view's extent is read; wide loads where base and strides are 16-byte aligned
 * (U8: 4-byte), element-wide range-checked loads otherwise. */
enum nconv_color_kind { NCONV_COLOR_NONE = 0, NCONV_COLOR_F32_PLANAR = 1, NCONV_COLOR_U8_INTERLEAVED = 2 };

typedef struct nconv_backproject {
    int B, H, W;
    int color_kind;                  /* enum nconv_color_kind; NONE with color == NULL            */
    const float* depth;
    long long depth_image_stride;    /* elements (ignored when B == 1)                            */
    long long depth_row_stride;      /* elements, >= W                                            */
    const float* conf;               /* NULL: no confidence gate                                  */
    long long conf_image_stride;
    long long conf_row_stride;
    const void* color;               /* NULL: no colour                                           */
    long long color_image_stride;    /* elements of the colour's type (ignored when B == 1)       */
    long long color_channel_stride;  /* F32_PLANAR only, >= H * row stride                        */
    long long color_row_stride;      /* >= W (F32_PLANAR) / >= 3 W (U8_INTERLEAVED)               */
    int reverse;                     /* != 0: the point's three colour bytes in reverse order     */
    float z_min;                     /* valid: z > z_min                                          */
    float z_max;                     /* ... && z <= z_max; 0 (with z_min >= 0): FLT_MAX           */
    float conf_min;                  /* ... && conf >= conf_min                                   */
    const float* k;                  /* (3, 3) or (B, 3, 3) fp32 row-major, on the device         */
    long long k_image_stride;        /* floats; 0: one camera for the batch                       */
} nconv_backproject;

/* The organised form for consumers that keep the image grid (normals, meshing, reprojection): xyz
 * (B, 3, H, W) contiguous fp32, planes x, y, z; a pixel that is not valid is NaN in all three.
 * color is ignored. One kernel, no workspace. */
int nconv_backproject_map(const nconv_backproject* d, float* xyz, void* stream);

/* The packed form robotics / mapping consumers take: the valid pixels' points in raster order inside
 * an image, images in batch order, identical on every run (no atomics: the order comes from a scan).
 *   xyz      (capacity, 3) fp32, interleaved
 *   rgb      (capacity, 3) uint8; NULL: skip (d->color is then not read); with rgb != NULL
 *            d->color must be given
 *   index    (capacity) int32 = (b * H + i) * W + j of each point; NULL: skip
 *   offsets  (B + 1) int32: image b's points are [offsets[b], offsets[b + 1]); offsets[B] is the TRUE
 *            number of valid pixels, also when it exceeds capacity: points of rank >= capacity are
 *            not written, so the caller detects truncation without a second run.
 * B * H * W must be < 2^31, and the B * H * ceil(W / 256) segments at most 2^24 (-EINVAL above).
 * workspace: nconv_backproject_workspace_bytes(B, H, W) bytes (0 for invalid sizes), 4-byte
 * aligned, overwritten. Three kernels on `stream` (count, scan, write), no host synchronisation, no
 * waiting between workgroups. xyz may be NULL when capacity is 0. */
size_t nconv_backproject_workspace_bytes(int B, int H, int W);
int nconv_backproject_points(const nconv_backproject* d, float* xyz, unsigned char* rgb, int* index,
                             long long capacity, int* offsets, void* workspace, size_t workspace_bytes,
                             void* stream);

/* ABI 27. An unordered LiDAR scan and a 3x4 projection -> the sparse depth plane S the models take,
 * the inverse of nconv_backproject_points and under the same convention (pixel centres at integer
 * coordinates, one fp32 rounding per operation). The reference has no counterpart: it reads S from
 * KITTI's velodyne_raw PNGs, rasterised offline. With PyTorch ops the same result is a matmul, three
 * elementwise passes and a boolean mask, a scatter_reduce_(amin) and a fix-up of the empty pixels,
 * with no defined winner between points that tie.
 * Inputs:
 *   points   fp32 rows of point_stride floats, point_stride >= 3 (and <= 2^20); only the first three
 *            floats (x, y, z) of a row are read: KITTI's .bin scans have point_stride 4, the xyz of
 *            nconv_backproject_points 3. 4-byte aligned; no byte outside
 *            [points, points + ((n_rows - 1) * point_stride + 3) * 4) is read.
 *   offsets  (B + 1) int32 on the device, non-decreasing, offsets[B] <= n_rows: image b owns the rows
 *            [offsets[b], offsets[b + 1]), the layout nconv_backproject_points emits. Rows from
 *            offsets[B] on (and below offsets[0]) are ignored. n_rows is a host value and sizes the
 *            grid; the offsets are never read on the host.
 *   m        fp32 row-major 3x4 projection of image b at m + b * m_image_stride, read on the device;
 *            m_image_stride = 0: one camera for the whole batch.
 * Per point p = (x, y, z), with a row r = (r0, r1, r2, r3) of m,
 *     dot(r, p) = ((r0 * x + r1 * y) + r2 * z) + r3
 * each operation one fp32 rounding in that order (no FMA), and
 *     a = dot(m[0], p), b = dot(m[1], p), c = dot(m[2], p),  u = a / c, v = b / c  (IEEE division),
 *     fj = rintf(u), fi = rintf(v)                                               (ties to even).
 * The point is valid iff
 *     c > z_min && c <= z_max && fj >= 0 && fj <= W - 1 && fi >= 0 && fi <= H - 1
 * all float comparisons made before any integer conversion, so NaN, +-inf and huge coordinates are
 * simply not valid. z_min must be >= 0; z_max = 0 means FLT_MAX, as in nconv_backproject.
 * Outputs:
 *   depth    (B, 1, H, W) contiguous fp32, overwritten entirely: depth[b][0][i][j] = the minimum c
 *            over the valid points of image b that land on (i, j), 0.0f where none lands.
 *   index    optional (B, H, W) int32: the row number in `points` of the winning point, -1 where the
 *            pixel is empty; among points with bit-equal c on one pixel the smallest row number wins.
 * Both are functions of the input alone: identical on every run, whatever order the hardware
 * executes in (an integer minimum over the bit pattern of c, which is positive and so orders as an
 * unsigned integer).
 * (the struct tag shares its name with the entry point, as nconv_frame_ingest's does: spell the type
 * `struct nconv_lidar_project` or nconv_lidar_project_desc) */
typedef struct nconv_lidar_project {
    int B, H, W;
    int point_stride;          /* floats per row, >= 3                                          */
    const float* points;       /* may be NULL when n_rows == 0                                  */
    long long n_rows;          /* rows in points, 0 <= n_rows < 2^31                            */
    const int* offsets;        /* (B + 1) int32, on the device                                  */
    const float* m;            /* (3, 4) or (B, 3, 4) fp32 row-major, on the device             */
    long long m_image_stride;  /* floats; 0: one camera for the batch                           */
    float z_min;               /* valid: c > z_min (>= 0)                                       */
    float z_max;               /* ... && c <= z_max; 0: FLT_MAX                                 */
} nconv_lidar_project_desc;

/* Without index: 0 (the z-buffer is the output plane itself). With index: 8 * B * H * W bytes, a
 * 64-bit key (bits(c) << 32 | row) per pixel. 0 for invalid sizes (B, H or W <= 0, B * H * W >= 2^31). */
size_t nconv_lidar_project_workspace_bytes(int B, int H, int W, int with_index);

/* Three kernels on `stream` (fill, scatter, resolve), no host synchronisation, no allocation, no
 * waiting between workgroups. index NULL: the workspace is not used. Otherwise workspace must hold
 * nconv_lidar_project_workspace_bytes(B, H, W, 1) bytes, 8-byte aligned; it is overwritten. depth and
 * index are 4-byte aligned. n_rows == 0 is legal: an all-zero plane, index all -1. -EINVAL before any
 * launch for a NULL descriptor / points (with n_rows > 0) / offsets / m / depth, B, H or W <= 0,
 * B * H * W >= 2^31, n_rows < 0 or >= 2^31, point_stride < 3 or > 2^20, m_image_stride < 0, z_min < 0
 * or NaN, z_max < z_min with z_max != 0 (or NaN), a workspace that is NULL, short or misaligned beside
 * an index, misaligned points, offsets, m, depth or index. */
int nconv_lidar_project(const struct nconv_lidar_project* d, float* depth, int* index, void* workspace,
                        size_t workspace_bytes, void* stream);

/* Added under ABI 27 (purely additive: two new entry points and one new struct, nothing existing
 * changes, so NCONV_ABI_VERSION stays 27). A depth plane -> the picture of it: uint8 (B, H, W, 3)
 * through a 256-entry colour table. Replaces the reference's save_depth arithmetic (utils.py:12-16:
 * min-max normalise on the host, cv2.applyColorMap(..., COLORMAP_INFERNO)); the builtin tables are the
 * 256 listed colours of matplotlib's maps times 255, rounded (tools/gen_colormaps.py), which is how
 * OpenCV's tables of the same names are defined. Parity with cv2 itself is not pinned by a test.
 * Per pixel value v of image b, every operation one fp32 rounding (no FMA):
 *   empty   iff v is not finite or v <= floor (floor = -inf: only the non-finite values)
 *   lo, hi  auto_range: the minimum and maximum of image b's non-empty source pixels; else vmin, vmax
 *   s       = 255.0f / (hi - lo)                                     (IEEE division)
 *   idx     = clamp((int)rintf((v - lo) * s), 0, 255)                (ties to even)
 *             the clamp is made on the float: a product beyond the int range saturates, NaN gives 0;
 *             hi <= lo: idx = 0 for every non-empty pixel
 * radius r > 0 (a sparse plane drawn as squares): an output pixel shows the smallest non-empty value of
 * its (2r + 1) x (2r + 1) window clipped at the image border, and is empty if the window holds none.
 * lo and hi always come from the source plane, not from the windows.
 * Output: out[b][i][j][0..2] = table[idx] (R, G, B; B, G, R with bgr) for a non-empty pixel; for an
 * empty one the background pixel's three bytes as they are (bgr does not reorder them), or, without a
 * background, empty_rgb (R, G, B; written B, G, R with bgr). The result is a function of the input
 * alone: identical on every run.
 * (the struct tag shares its name with the entry point: spell the type `struct nconv_depth_colorize`
 * or nconv_depth_colorize_desc) */
typedef struct nconv_depth_colorize {
    int B, H, W;
    int radius;                         /* 0 .. 4                                                    */
    const float* depth;                 /* fp32 view: B planes of H rows of W, 4-byte aligned        */
    long long image_stride;             /* elements; ignored when B == 1                             */
    long long row_stride;               /* elements, >= W (a cropped DNET output works)              */
    const unsigned char* lut;           /* 256 x 3 uint8 R, G, B on the device, or NULL: cmap_id     */
    int cmap_id;                        /* 0 inferno, 1 magma, 2 viridis, 3 turbo, 4 gray            */
    int auto_range;                     /* nonzero: per-image min / max (needs the workspace)        */
    float vmin, vmax;                   /* lo, hi when auto_range == 0                               */
    float floor;                        /* empty: v <= floor; -INFINITY: none but non-finite values  */
    int bgr;                            /* nonzero: write B, G, R                                    */
    const unsigned char* background;    /* optional interleaved uint8 (B, H, W, 3) view              */
    long long background_image_stride;  /* bytes; ignored when B == 1                                */
    long long background_row_stride;    /* bytes, >= 3 * W                                           */
    unsigned char empty_rgb[3];         /* an empty pixel without a background                       */
} nconv_depth_colorize_desc;

/* 8 * B bytes: a minimum and a maximum key per image. 0 for B <= 0. */
size_t nconv_depth_colorize_workspace_bytes(int B);

/* out: (B, H, W, 3) contiguous uint8, any alignment, overwritten entirely. With auto_range three
 * kernels on `stream` (range reset, range reduce, map) and workspace must hold
 * nconv_depth_colorize_workspace_bytes(B) bytes, 8-byte aligned (overwritten); with a fixed range one
 * kernel, and the workspace is not used. No host synchronisation, no allocation, no waiting between
 * workgroups. -EINVAL before any launch for a NULL descriptor / depth / out, B, H or W <= 0,
 * B * H * W >= 2^31, radius outside 0..4, cmap_id outside 0..4 beside a NULL lut, NaN vmin or vmax
 * without auto_range, NaN floor, a workspace that is NULL, short or misaligned with auto_range, depth
 * not 4-byte aligned, and a depth or background view whose strides are smaller than its rows / images
 * or whose image spans 2^31 bytes or more. */
int nconv_depth_colorize(const struct nconv_depth_colorize* d, unsigned char* out, void* workspace,
                         size_t workspace_bytes, void* stream);

/* Added under ABI 27 (purely additive: two new entry points and one new struct, nothing existing
 * changes, so NCONV_ABI_VERSION stays 27). Surface normals of a depth map on the image grid, from the
 * same descriptor nconv_backproject_map takes (checked in the same way; color is ignored): what
 * point-to-plane ICP, meshing, ground segmentation and shaded rendering expect beside the points. With
 * PyTorch ops the same result is about fifteen elementwise passes over (B, 3, H, W).
 * Every arithmetic operation below is one fp32 rounding in the stated order, no FMA contraction;
 * division and square root are IEEE (correctly rounded). For image b, pixel (i, j):
 *   V(i, j)   the pixel is inside the image and valid by nconv_backproject's rule
 *             (z > z_min && z <= z_max && (conf == NULL || conf >= conf_min)); a pixel outside the
 *             image is not valid whatever z_min is
 *   P(i, j)   nconv_backproject's point (x, y, z), bit for bit
 * A centre c with V false has no normal. Otherwise, with z its depth,
 *   tol       = jump_abs + jump_rel * z                       (one multiply, one add)
 *   usable(n) = V(n) && (gate off || fabsf(z_n - z) <= tol)   (comparisons: a NaN is not usable)
 *               the gate is off when jump_rel == 0 && jump_abs == 0
 *   tu        from R = (i, j + 1) and L = (i, j - 1): both usable P(R) - P(L); only R: P(R) - P(c);
 *             only L: P(c) - P(L); neither: no normal
 *   tv        from D = (i + 1, j) and T = (i - 1, j) by the same rule, D in the role of R
 *   c = tv x tu:  cx = tv.y * tu.z - tv.z * tu.y,  cy = tv.z * tu.x - tv.x * tu.z,
 *                 cz = tv.x * tu.y - tv.y * tu.x      (a fronto-parallel surface gives (0, 0, -1))
 *   d         = (cx * P.x + cy * P.y) + cz * P.z; d > 0: c = -c, so that n . P <= 0 (towards the camera)
 *   l         = sqrtf((cx * cx + cy * cy) + cz * cz); the pixel has a normal iff l > 0 && l < INFINITY
 *   n         = (cx / l, cy / l, cz / l)
 * H == 1 or W == 1 is legal and yields no normal anywhere. The result is a function of the input
 * alone: identical on every run. */
typedef struct nconv_normals_opts {
    float jump_rel, jump_abs;      /* both 0: no discontinuity gate */
    unsigned char empty_rgb[3];    /* picture: a pixel without a normal */
} nconv_normals_opts;              /* NULL: all zero */

/* Either or both of (NULL: skip)
 *   normals  (B, 3, H, W) contiguous fp32, planes nx, ny, nz; NaN in all three where the pixel has no
 *            normal. 4-byte aligned.
 *   image    (B, H, W, 3) contiguous uint8, any alignment: the camera-space normal picture,
 *            R = q(nx), G = q(-ny), B = q(-nz) with q(t) = clamp(rintf((t * 0.5f + 0.5f) * 255.0f), 0, 255)
 *            and (0.5f - t * 0.5f) for the negated channels; empty_rgb where there is no normal.
 * One kernel on `stream`, no workspace, no host synchronisation; the picture is made without the fp32
 * map reaching memory. No byte outside a view's extent is read. -EINVAL before any launch for whatever
 * nconv_backproject_map refuses in d, both outputs NULL, a NaN or negative jump_rel or jump_abs, and
 * normals not 4-byte aligned. */
int nconv_depth_normals(const nconv_backproject* d, const nconv_normals_opts* o, float* normals,
                        unsigned char* image, void* stream);

/* The same normals for the rows of a packed cloud (index and offsets as nconv_backproject_points wrote
 * them for the same d): normals[r] = three fp32, interleaved, the normal of pixel index[r] =
 * (b * H + i) * W + j for every r < min(offsets[B], capacity), and (0, 0, 0) where that pixel has no
 * normal (the PLY convention) or index[r] lies outside [0, B * H * W), for which nothing is read. Rows
 * from min(offsets[B], capacity) on are not written. offsets[B] is read on the device; capacity is a
 * host value and sizes the grid. One kernel, no workspace, no host synchronisation. capacity == 0 is
 * legal and launches nothing. -EINVAL before any launch for whatever nconv_backproject_map refuses in
 * d, a NaN or negative jump_rel or jump_abs, a negative capacity, a NULL index, offsets or normals
 * beside capacity > 0, and index, offsets or normals not 4-byte aligned. */
int nconv_depth_normals_points(const nconv_backproject* d, const nconv_normals_opts* o, const int* index,
                               const int* offsets, long long capacity, float* normals, void* stream);

/* Added under ABI 27 (purely additive: two new entry points and one new struct, nothing existing
 * changes, so NCONV_ABI_VERSION stays 27). A depth plane -> a random sparse subset of it with an exact
 * number of samples per image: the training input of the reference (DataLoader_NYU.preprocess_depth:
 * randperm, gather / scatter, mask) on the device, the "N random samples" protocol, and thinning a
 * LiDAR plane to a budget. The result is a function of (input, seed, draw) alone: identical on every
 * run and for every launch geometry. It does not reproduce torch.randperm's stream.
 * For image b and pixel p = row * W + col (the logical pixel number, never a memory offset, so that a
 * cropped view samples like its contiguous copy):
 *   words      (w0, w1, w2, w3) = Philox4x32-10(counter = (p, b, draw, 0), key = (seed_lo, seed_hi))
 *              (csrc/philox.h), with state = {seed_lo, seed_hi, draw} read from device memory: a
 *              captured graph is replayed with a fresh draw by changing state[2]. A call never writes it.
 *   candidate  iff (mask == NULL || mask byte != 0) && (all_pixels || (d > floor && d <= FLT_MAX)), d the
 *              source value (comparisons: a NaN is no candidate). C_b: the candidates of image b.
 *   target     n_b = C_b                                      NCONV_SPARSIFY_ALL
 *                    min(n, C_b)                              NCONV_SPARSIFY_COUNT
 *                    min(max(n_dev[b], 0), C_b)               NCONV_SPARSIFY_COUNT_DEV
 *                    (int)floor((double)keep * (double)C_b)   NCONV_SPARSIFY_FRACTION
 *   kept       the n_b candidates that are smallest under the order (w0 & key_mask, p). The pair is
 *              unique, so the set is fully determined. key_mask is 0xffffffff in ordinary use; smaller
 *              masks force ties onto p, and key_mask = 0 keeps the first n_b candidates in raster order.
 *   noise      a kept pixel is noisy iff w1 < noise_threshold (0: no noise; for a share f of the kept
 *              pixels the host passes floor(f * 2^32) clamped to [0, 2^32 - 1]). Then
 *                u = (float)(w2 >> 8) * 2^-24,  s = 2 u - 1 (exact),  r = noise_amp * s,  t = d * r,
 *                out = d + t
 *              the last three one fp32 rounding each, no FMA: the reference's flat[idx] += flat[idx] *
 *              noise. Where that result is a NaN (d not finite, with all_pixels) its sign and payload
 *              are not specified. Noise is Bernoulli per pixel; the reference perturbs an exact count.
 *   output     a kept pixel that is not noisy holds d bit for bit; every pixel that is not kept +0.0f.
 * (the struct tag shares its name with the entry point: spell the type `struct nconv_depth_sparsify`
 * or nconv_depth_sparsify_desc) */
enum nconv_sparsify_mode {
    NCONV_SPARSIFY_ALL = 0,
    NCONV_SPARSIFY_COUNT = 1,
    NCONV_SPARSIFY_COUNT_DEV = 2,
    NCONV_SPARSIFY_FRACTION = 3
};

typedef struct nconv_depth_sparsify {
    int B, H, W;
    int mode;                       /* enum nconv_sparsify_mode                                   */
    const float* src;               /* fp32 view: B planes of H rows of W, 4-byte aligned         */
    long long src_image_stride;     /* elements; ignored when B == 1                              */
    long long src_row_stride;       /* elements, >= W                                             */
    const unsigned char* mask;      /* optional uint8 view; NULL: every pixel passes              */
    long long mask_image_stride;    /* bytes; 0: one mask for the batch                           */
    long long mask_row_stride;      /* bytes, >= W                                                */
    const unsigned* state;          /* {seed_lo, seed_hi, draw} on the device, 4-byte aligned     */
    const int* n_dev;               /* (B) int32 on the device: COUNT_DEV                         */
    int n;                          /* COUNT, >= 0                                                */
    float keep;                     /* FRACTION, 0 <= keep <= 1                                   */
    int all_pixels;                 /* nonzero: floor is not applied (the reference's NYU rule)   */
    float floor;                    /* candidate: d > floor                                       */
    unsigned key_mask;              /* 0xffffffff; see `kept`                                     */
    unsigned noise_threshold;       /* noisy: w1 < noise_threshold                                */
    float noise_amp;                /* r = noise_amp * s                                          */
} nconv_depth_sparsify_desc;

/* Per image six 2048-bin digit histograms and six selection states. 0 for invalid sizes (B, H or
 * W <= 0, B * H * W >= 2^31). */
size_t nconv_depth_sparsify_workspace_bytes(int B, int H, int W);

/* dst: fp32 view of B planes of H rows of W with its own strides in elements, overwritten entirely; it
 * may be src itself (same pointer, same strides: in place), any other overlap of the two extents is
 * refused. kept: optional (B) int32 = n_b. workspace: nconv_depth_sparsify_workspace_bytes(B, H, W)
 * bytes, 8-byte aligned, overwritten; nothing in it is carried from one call to the next.
 * Always eight kernels on `stream` whatever the data, the mode and n: one that zeroes the histograms,
 * then the selection, a radix select over the 64-bit composite (w0 & key_mask) << 32 | p in six passes of
 * 11, 11, 11, 11, 10 and 10 bits from the top (per-image histograms, private in LDS, merged with integer
 * atomics: independent of the order of execution), each pass resolving the previous pass's bucket first,
 * then the pass that writes dst. No host synchronisation, no allocation, no waiting between workgroups: capturable.
 * -EINVAL before any launch for a NULL descriptor / src / dst / state, B, H or W <= 0,
 * B * H * W >= 2^31, a row stride below W, images that overlap (an image stride below H * row stride;
 * the mask's may be 0), an unknown mode, COUNT_DEV without n_dev, a negative n, keep outside [0, 1] or
 * NaN, a workspace that is NULL, short or misaligned, src / dst / state / n_dev / kept not 4-byte
 * aligned, and a dst that overlaps src without being src. */
int nconv_depth_sparsify(const struct nconv_depth_sparsify* d, float* dst, long long dst_image_stride,
                         long long dst_row_stride, int* kept, void* workspace, size_t workspace_bytes,
                         void* stream);

/* Added under ABI 27 (purely additive: one new entry point and one new struct, nothing existing
 * changes, so NCONV_ABI_VERSION stays 27). Occluded LiDAR returns taken out of a sparse depth plane.
 * The scanner does not sit where the camera sits (KITTI: about 8 cm above and 27 cm behind cam0), so
 * beside every foreground silhouette the projected scan holds background returns the camera cannot
 * see, between the foreground returns. nconv_lidar_project resolves collisions on one pixel only, and
 * KITTI's velodyne_raw PNGs hold such returns too. The remedy is the usual local window test: a return
 * is dropped when enough clearly nearer returns lie next to it.
 * Every arithmetic operation below is one fp32 rounding in the stated order, no FMA contraction. For
 * image b and pixel p = (i, j) with value v_p:
 *   valid(p)    v_p is finite and v_p > floor (floor = -INFINITY: every finite value is valid); the
 *               "empty" rule of nconv_depth_colorize
 *   lim(q)      = v_q + (jump_abs + jump_rel * v_q)       (one multiply, two adds), for valid q
 *   window(p)   the pixels q != p with |i_q - i_p| <= rh and |j_q - j_p| <= rw that lie inside the
 *               image: the window is clipped at the border, and a pixel outside the image is no
 *               candidate whatever floor is
 *   support(p)  the number of valid q of window(p) with v_p > lim(q)   (a strict float comparison: a
 *               NaN or +inf lim supports nothing)
 *   removed(p)  valid(p) && support(p) >= min_support
 *   dst[p]      v_p bit for bit where p is valid and not removed, +0.0f everywhere else (removed,
 *               empty and non-finite pixels)
 * rh = rw = 0 removes nothing; a min_support larger than the window is legal and removes nothing. The
 * result is a function of the input alone: identical on every run. The source is only read.
 * What the rule cannot avoid: a visible background return just outside a silhouette has nearer returns
 * in its window too and is dropped as well; on the road surface a tall window with a small jump_abs /
 * jump_rel removes far ground returns in favour of the nearer scan line below them; min_support > 1
 * keeps one stray near return (dust, rain) from clearing a window of good ones. Nobody has measured
 * parameter values on KITTI.
 * (the struct tag shares its name with the entry point: spell the type `struct nconv_depth_occlusion`
 * or nconv_depth_occlusion_desc) */
typedef struct nconv_depth_occlusion {
    int B, H, W;
    int rh, rw;                     /* window half-heights / half-widths, 0 .. 16 (up to 33 x 33)  */
    int min_support;                /* >= 1                                                        */
    const float* src;               /* fp32 view: B planes of H rows of W, 4-byte aligned          */
    long long src_image_stride;     /* elements; ignored when B == 1                               */
    long long src_row_stride;       /* elements, >= W                                              */
    float jump_abs, jump_rel;       /* >= 0, not NaN                                               */
    float floor;                    /* valid: v > floor; not NaN                                   */
} nconv_depth_occlusion_desc;

/* dst: fp32 view of B planes of H rows of W with its own strides in elements, overwritten entirely.
 * It must not overlap src: neighbours are read, so there is no in-place operation, and the host
 * compares the two byte extents. Optional outputs (NULL: skip):
 *   removed  (B, H, W) contiguous uint8, 1 where the pixel is removed and 0 elsewhere, written entirely
 *   index    (B, H, W) contiguous int32, updated in place: -1 where the pixel is removed or not valid,
 *            left alone elsewhere. The index plane of nconv_lidar_project, so that the caller can name
 *            the scan rows that were dropped.
 *   counts   (B, 2) int32 = {valid pixels, removed pixels} of every image (integer atomics: the same
 *            on every run)
 * One kernel on `stream`, preceded by one small kernel that zeroes counts when counts is given. No
 * workspace, no host synchronisation, no allocation, no waiting between workgroups: capturable. No
 * byte outside the source view's extent is read. A workgroup stages a 32 x 64 tile with its halo in
 * LDS, lists the tile's valid pixels and shares each one's window across lanes.
 * -EINVAL before any launch for a NULL descriptor / src / dst, B, H or W <= 0, B * H * W >= 2^31, rh or
 * rw outside 0..16, a negative or NaN jump_abs or jump_rel, a NaN floor, min_support < 1, src / dst /
 * index / counts not 4-byte aligned, a src or dst view whose strides are smaller than its rows /
 * images or whose image spans 2^31 bytes or more, and a dst whose extent overlaps src's. */
int nconv_depth_occlusion(const struct nconv_depth_occlusion* d, float* dst, long long dst_image_stride,
                          long long dst_row_stride, unsigned char* removed, int* index, int* counts,
                          void* stream);

/* Added under ABI 27 (purely additive: one new entry point and two new structs, nothing existing
 * changes, so NCONV_ABI_VERSION stays 27). The training augmentation of a depth-completion batch: one
 * random crop window and one horizontal flip per image, applied alike to every tensor of the batch, the
 * intrinsics rewritten to match, photometric jitter on the RGB, and a report of what was drawn. These
 * are not torchvision's ColorJitter semantics: contrast pivots on a constant, not on the image mean,
 * and there is no hue. No resampling of any kind: sparse depth cannot be interpolated honestly.
 * Sources (each optional; all of source size (H, W), batch B, unit-stride rows, strides in elements
 * unless stated): rgb fp32 (B, 3, H, W) with image, channel and row strides; plane[0..2] fp32
 * single-channel planes (sparse depth, ground truth, one spare) with image and row strides; mask uint8
 * (B, H, W) with strides in bytes and no alignment requirement, image stride 0: one mask for the batch;
 * k fp32 (B, 3, 3) contiguous. Outputs: contiguous tensors of the output size (h, w), 1 <= h <= H and
 * 1 <= w <= W ((B, 3, h, w), (B, h, w)), each overwritten entirely; k_out (B, 3, 3); optional params
 * (B, 4) int32 {y0, x0, flip, 0}; optional gains (B, 5) fp32 {g_b, g_c, gain_0, gain_1, gain_2}.
 * For image b:
 *   words      (w0, w1, w2, w3) = Philox4x32-10(counter = (b, 0, draw, 1), key = (seed_lo, seed_hi))
 *              (j0, j1, j2, j3) = Philox4x32-10(counter = (b, 1, draw, 1), key = (seed_lo, seed_hi))
 *              (csrc/philox.h), state = {seed_lo, seed_hi, draw} read from device memory and never
 *              written by the call. The last counter word 1 keeps these streams apart from
 *              nconv_depth_sparsify's (p, b, draw, 0).
 *   window     per axis its own mode; y0 from (mode_y, w0, H, h), x0 alike from (mode_x, w1, W, w):
 *                NCONV_AUGMENT_RANDOM   (uint32)(((uint64)w0 * (uint64)(H - h + 1)) >> 32)
 *                NCONV_AUGMENT_CENTER   (H - h) / 2, integer division
 *                NCONV_AUGMENT_MIN      0
 *                NCONV_AUGMENT_MAX      H - h (KITTI's "keep the bottom rows")
 *   flip       (uint64)w2 < flip_threshold, flip_threshold in 0 .. 2^32: for a probability p the host
 *              passes floor(p * 2^32) clamped to that range, so 0 never flips and 2^32 always flips.
 *   geometry   out[b][..][i][j] = src[b][..][y0 + i][flip ? x0 + (w - 1 - j) : x0 + j] for every plane,
 *              the mask and the RGB channels: a bit-for-bit copy, NaNs and payloads included. No byte
 *              outside a source view's extent is read.
 *   intrinsics each operation one fp32 rounding:
 *                cx1 = k[0][2] - (float)x0,  cy1 = k[1][2] - (float)y0
 *                k_out[0][2] = flip ? (float)(w - 1) - cx1 : cx1,  k_out[1][2] = cy1
 *              and the other seven entries copied bit for bit.
 *   jitter     RGB only, and skipped entirely when brightness == contrast == color == 0: the RGB is then
 *              a bit-for-bit copy without a clamp and the gains are reported as 1. Otherwise, with
 *              u(x) = (float)(x >> 8) * 2^-24 and s(x) = 2 u(x) - 1 (both exact),
 *                g_b = 1 + brightness * s(j0),  g_c = 1 + contrast * s(j1),
 *                gain_0 = 1 + color * s(w3),  gain_1 = 1 + color * s(j2),  gain_2 = 1 + color * s(j3)
 *              (one multiply and one add each), and for a value v of channel plane c, in this order, one
 *              fp32 rounding per operation and no FMA contraction:
 *                a = v * g_b;  a = a * gain_c;  a = a - pivot;  a = a * g_c;  a = a + pivot;
 *                out = fminf(fmaxf(a, 0.0f), rgb_max)
 *              the clamp made by comparisons (a > 0 ? a : 0, then a < rgb_max ? a : rgb_max), so that
 *              -0.0 comes out as +0.0. A NaN v with jitter on gives an unspecified result. The usual
 *              values are pivot = 127.5 and rgb_max = 255.
 * The result is a function of (inputs, seed, draw) alone: identical on every run and for every launch
 * geometry. csrc/augment_params.h holds the draw as code a host program can compile.
 * (the struct tag shares its name with the entry point: spell the type `struct nconv_frame_augment`
 * or nconv_frame_augment_desc) */
enum nconv_augment_crop {
    NCONV_AUGMENT_RANDOM = 0,
    NCONV_AUGMENT_CENTER = 1,
    NCONV_AUGMENT_MIN = 2,
    NCONV_AUGMENT_MAX = 3
};

typedef struct nconv_augment_plane {
    const float* src;               /* NULL: absent; fp32 view, 4-byte aligned                     */
    long long image_stride;         /* elements; ignored when B == 1                               */
    long long row_stride;           /* elements, >= W                                              */
    float* out;                     /* (B, 1, h, w) contiguous                                     */
} nconv_augment_plane;

typedef struct nconv_frame_augment {
    int B, H, W;                    /* batch and source size                                       */
    int h, w;                       /* output size                                                 */
    int mode_y, mode_x;             /* enum nconv_augment_crop                                     */
    unsigned long long flip_threshold; /* 0 .. 2^32                                                */
    const unsigned* state;          /* {seed_lo, seed_hi, draw} on the device, 4-byte aligned      */
    const float* rgb;               /* NULL: absent; fp32 (B, 3, H, W) view                        */
    long long rgb_image_stride;     /* elements; ignored when B == 1                               */
    long long rgb_channel_stride;   /* elements                                                    */
    long long rgb_row_stride;       /* elements, >= W                                              */
    float* rgb_out;                 /* (B, 3, h, w) contiguous                                     */
    nconv_augment_plane plane[3];
    const unsigned char* mask;      /* NULL: absent; uint8 view, any alignment                     */
    long long mask_image_stride;    /* bytes; 0: one mask for the batch                            */
    long long mask_row_stride;      /* bytes, >= W                                                 */
    unsigned char* mask_out;        /* (B, 1, h, w) contiguous                                     */
    const float* k;                 /* NULL: absent; (B, 3, 3) contiguous                          */
    float* k_out;                   /* (B, 3, 3)                                                   */
    int* params;                    /* optional (B, 4) {y0, x0, flip, 0}                           */
    float* gains;                   /* optional (B, 5) {g_b, g_c, gain_0, gain_1, gain_2}          */
    float brightness, contrast, color; /* amplitudes in [0, 1]                                     */
    float pivot, rgb_max;           /* 127.5 and 255 in ordinary use                               */
} nconv_frame_augment_desc;

/* One kernel on `stream` for every tensor of the batch: the grid's z dimension enumerates images, y the
 * tensor slots (each RGB channel, each plane, the mask) and x groups of four output pixels of a row, so
 * the draw of an image is uniform over a workgroup. A lane stores its four pixels as 16 bytes where the
 * address allows, reads its four source pixels (reversed under a flip) at their 4-byte alignment, and
 * the first workgroup of an image writes k_out, params and gains. No workspace, no atomics, no host
 * synchronisation, no allocation, no waiting between workgroups: capturable.
 * -EINVAL before any launch for a NULL descriptor or state; no source at all; a source without its
 * output or an output without its source (k without k_out included); B, H, W, h or w <= 0; h > H or
 * w > W; B * 3 * H * W >= 2^31; a row stride below W, or images or channels that overlap (an image stride
 * below the image's extent, a channel stride below H * row stride; the mask's image stride may be 0);
 * an unknown mode; flip_threshold > 2^32; an amplitude that is NaN or outside [0, 1]; a NaN pivot or
 * rgb_max, or rgb_max < 0; fp32 / int32 pointers or state not 4-byte aligned; and any output extent
 * that overlaps a source extent (state counts as a source). */
int nconv_frame_augment(const struct nconv_frame_augment* d, void* stream);

/* Added under ABI 27 (purely additive: two new entry points and one new struct, nothing existing
 * changes, so NCONV_ABI_VERSION stays 27). Sparsification curves of a confidence plane (Ilg et al. 2018):
 * remove the least confident valid pixels step by step and sum the error of the rest, beside the oracle
 * that removes the largest errors first. pred, gt and conf are B planes (H, W) of fp32, each with image
 * and row strides in elements (cropped views, and a first element that is not 16-byte aligned, are
 * allowed, as in nconv_depth_metrics). Per image b, with pixel number p = row * W + col:
 *   valid      as in nconv_depth_metrics: gt > 0, gt >= gt_min, gt <= gt_max (a bound of 0 is absent);
 *              n_b = the number of valid pixels.
 *   terms      P = pred clamped into [clamp_lo, clamp_hi] by comparisons (a bound of 0 is absent; a NaN
 *              stays NaN); e = P - gt, a = |e|, q = e * e, in fp32 with no contraction.
 *   conf key   bits = as_uint(conf); u = bits ^ (bits >> 31 ? 0xFFFFFFFF : 0x80000000), which preserves
 *              the order of the floats (-0.0 ranks below +0.0). With uncertainty != 0 the plane is an
 *              uncertainty (larger is worse) and the key is ~u. A NaN conf has the key 0 under either
 *              reading: it is removed first.
 *   oracle key v = ~as_uint(a): the largest error first, a NaN error before +inf.
 *   order      for each ranking o (0: conf key, 1: oracle key) the valid pixels sorted by ascending key,
 *              ties broken by ascending p. No two elements compare equal, so the order is unique.
 *   curve      steps = J in [1, 1024]; for j = 0 .. J-1, k_j = floor(j * n_b / J) in 64-bit integers, the
 *              kept set is positions k_j .. n_b - 1 of the order, and
 *                curves[b][o][j] = { n_b - k_j, sum of a, sum of q } over the kept set (three doubles).
 *              n_b == 0 gives rows of zeros.
 * The count is exact. The summation order is fixed: the sorted positions are cut into chunks of 256; the
 * terms of a chunk, as doubles, are thread values t = 0 .. 255 of a tree T that adds values t and t ^ 32,
 * then ^ 16, ^ 8, ^ 4, ^ 2, ^ 1 inside each group of 64, then ((g0 + g1) + g2) + g3 over the four groups;
 * absent positions count as +0.0. With c = floor(k_j / 256), thread value t for curve point j is the term at
 * position 256 c + t where that lies in [k_j, n_b), else 0, plus the T-sums of chunks c + 1 + t,
 * c + 1 + t + 256, .. in that order; the point is T over those 256 values. The same input gives the same
 * bits on every run. No floating-point atomics, no global atomics.
 * curves: (B, 2, J, 3) doubles, 8-byte aligned, overwritten. order: optional (B, 2, H * W) int32;
 * order[b][o][0 .. n_b) holds the pixel numbers in removal order, the rest is -1; NULL skips it.
 * The sort is a segmented (image x ranking), stable, least-significant-digit radix sort of (key, p) pairs
 * with 8-bit digits; invalid pixels are left out by a raster-order compaction beforehand, which is also
 * what makes p the tie-break. Twelve launches on `stream` whatever the data, n_b and order; no host
 * synchronisation, no allocation: capturable. Every buffer lives in the workspace (8-byte aligned,
 * about 40 bytes per pixel of the batch).
 * -EINVAL before any launch for a NULL descriptor, plane or curves; B, H or W <= 0; steps outside
 * [1, 1024]; H * W >= 2^31 (pixel numbers are int32) or B * H * W >= 2^31; a view whose row stride is below W,
 * whose image stride is below H * row stride, or whose extent ((H - 1) * row stride + W) * 4 reaches 2^31
 * bytes ("plane too large"); a negative or NaN bound, gt_min > gt_max, clamp_lo > clamp_hi; planes or order
 * not 4-byte aligned, curves not 8-byte aligned; a workspace that is NULL, too small or not 8-byte aligned.
 * (the struct tag shares its name with the entry point: spell the type `struct nconv_depth_sparsification`
 * or nconv_depth_sparsification_desc) */
#define NCONV_SPARSIFICATION_MAX_STEPS 1024
typedef struct nconv_depth_sparsification {
    int B, H, W;
    int steps;                      /* J: 1 .. 1024                                                */
    const float* pred;              /* fp32 views, 4-byte aligned                                  */
    long long pred_image_stride;    /* elements; ignored when B == 1                               */
    long long pred_row_stride;      /* elements, >= W                                              */
    const float* gt;
    long long gt_image_stride;
    long long gt_row_stride;
    const float* conf;
    long long conf_image_stride;
    long long conf_row_stride;
    float gt_min, gt_max;           /* validity window of gt; 0: absent                            */
    float clamp_lo, clamp_hi;       /* clamp window of pred; 0: absent                             */
    int uncertainty;                /* != 0: conf is an uncertainty, the largest is removed first  */
    double* curves;                 /* (B, 2, J, 3)                                                */
    int* order;                     /* optional (B, 2, H * W)                                      */
} nconv_depth_sparsification_desc;

/* 0 for extents or steps that the call itself refuses. */
size_t nconv_depth_sparsification_workspace_bytes(int B, int H, int W, int steps);
int nconv_depth_sparsification(const struct nconv_depth_sparsification* d, void* workspace, size_t workspace_bytes,
                               void* stream);

/* Added under ABI 27 (purely additive: one new entry point and one new struct, nothing existing
 * changes, so NCONV_ABI_VERSION stays 27). Classical depth completion of a sparse depth plane: IP-Basic
 * (Ku, Harakeh, Waslander, "In Defense of Classical Image Processing: Fast Depth Completion on the CPU",
 * CRV 2018), its fill_in_fast made total (every input bit pattern has a defined result) and
 * deterministic. The non-learned baseline beside the NConv networks, a pre-densifier, a quick picture.
 * Every arithmetic operation below is one fp32 rounding in the stated order. T = 0.1f. In the inverted
 * domain a pixel is valid iff v > T and empty iff v < T; as in the original, v == T is neither. For
 * image b and pixel p with source value d_p:
 *   0. invert   sample(p) holds when d_p is finite, d_p > T and (max_depth - d_p) > T. Where sample(p)
 *               holds, v0 = max_depth - d_p; everywhere else v0 = +0.0f (NaN, +-inf, negatives, -0, too
 *               small and too far values). From here on every value is finite and >= 0.
 *   1. dilate   v1 = max of v0 over the in-image pixels of the kernel footprint, size s in {3, 5, 7},
 *               r = s / 2: NCONV_IPBASIC_FULL |dy| <= r, |dx| <= r; NCONV_IPBASIC_CROSS dy == 0 || dx == 0
 *               within r; NCONV_IPBASIC_DIAMOND |dy| + |dx| <= r. Pixels outside the image take no part in
 *               any dilation.
 *   2. close    v2 = erode(dilate(v1, full 5), full 5); erode is the min over the in-image window
 *               pixels: pixels outside the image take no part.
 *   3. fill     v3 = empty(v2) ? dilate(v2, full 7) : v2
 *   4. only with extrapolate: per image and column x, top(x) = the smallest row y with
 *               valid(v3[y, x]), 0 if the column has none;
 *               v3e[y, x] = y < top(x) ? v3[top(x), x] : v3[y, x];
 *               v4 = empty(v3e) ? dilate(v3e, full 31) : v3e. Without extrapolate, v4 = v3.
 *   5. median   (if on) v5[p] = the 13th smallest of the 25 values of the 5 x 5 window of v4, coordinates
 *               clamped to the image (replicate border), at every pixel. All inputs are finite and >= 0,
 *               so the selection is exact. Off: v5 = v4.
 *   6. blur     (NCONV_IPBASIC_BLUR_GAUSSIAN) separable, weights w = {0.0625, 0.25, 0.375, 0.25, 0.0625}
 *               (OpenCV's fixed 5-tap kernel for ksize 5, sigma 0); the horizontal pass first into h,
 *               then the vertical pass over h, each (((w0*a0 + w1*a1) + w2*a2) + w3*a3) + w4*a4, five
 *               products and four sums, each rounded on its own. The products by 0.0625 and 0.25 are
 *               exact, the one by 0.375 = 3 * 2^-3 is not (3 a needs two more bits than a), so
 *               contracting to FMA does change bits: no contraction. Border reflect-101
 *               (-1 -> 1, -2 -> 2, n -> n - 2, n + 1 -> n - 3), folded until inside; a dimension of 1
 *               maps every tap to 0. v6 = valid(v5) ? blurred : v5. NCONV_IPBASIC_BLUR_NONE: v6 = v5.
 *               (The upstream script's bilateral blur needs exp and is not offered.)
 *   7. back     out = valid(v6) ? max_depth - v6 : +0.0f; with keep_samples,
 *               out = sample(p) ? d_p (bit for bit) : that. Without keep_samples IP-Basic does not
 *               preserve its input samples: the median and the blur move them.
 * The result is a function of the input alone: identical on every run. The source is only read.
 * (the struct tag shares its name with the entry point: spell the type `struct nconv_depth_ipbasic`
 * or nconv_depth_ipbasic_desc) */
enum nconv_ipbasic_kernel {
    NCONV_IPBASIC_FULL = 0,
    NCONV_IPBASIC_CROSS = 1,
    NCONV_IPBASIC_DIAMOND = 2
};
enum nconv_ipbasic_blur {
    NCONV_IPBASIC_BLUR_NONE = 0,
    NCONV_IPBASIC_BLUR_GAUSSIAN = 1
};

typedef struct nconv_depth_ipbasic {
    int B, H, W;
    const float* src;               /* fp32 view: B planes of H rows of W, 4-byte aligned          */
    long long src_image_stride;     /* elements; ignored when B == 1                               */
    long long src_row_stride;       /* elements, >= W                                              */
    float max_depth;                /* finite, > 2 T (100 in ordinary use)                         */
    int kernel_shape;               /* enum nconv_ipbasic_kernel (diamond in ordinary use)         */
    int kernel_size;                /* 3, 5 or 7 (5 in ordinary use)                               */
    int extrapolate;                /* != 0: stage 4                                               */
    int median;                     /* != 0: stage 5                                               */
    int blur;                       /* enum nconv_ipbasic_blur                                     */
    int keep_samples;               /* != 0: the input samples come out bit for bit                */
} nconv_depth_ipbasic_desc;

/* dst: fp32 view of B planes of H rows of W with its own strides in elements, overwritten entirely.
 * It must not overlap src: neighbours are read, so there is no in-place operation, and the host
 * compares the two byte extents. Workspaces, needed with extrapolate only (else they may be NULL and
 * are not touched): work_plane (B, H, W) contiguous fp32 (v3), work_top (B, W) int32 (top(x)), both
 * overwritten, neither overlapping src or dst.
 * Without extrapolate one kernel on `stream`: a workgroup stages a 64 x 64 tile and its halo of 14 in
 * LDS, runs stages 0 to 7 between two LDS buffers and writes the tile once. With extrapolate three: one
 * that resets work_top, stages 0 to 3 into work_plane with top(x) taken by an integer atomicMin on the
 * row number (order-free), and the extrapolated read, the 31 x 31 fill and stages 5 to 7 from a tile
 * with a halo of 19. No float atomics, no host synchronisation, no allocation, no waiting between
 * workgroups: capturable. No byte outside the source view's extent is read.
 * -EINVAL before any launch for a NULL descriptor / src / dst, B, H or W <= 0, B * H * W >= 2^31, an
 * unknown kernel_shape, kernel_size or blur, a max_depth that is not finite or <= 2 T, src / dst /
 * work_plane / work_top not 4-byte aligned, a src or dst view whose strides are smaller than its rows /
 * images or whose image spans 2^31 bytes or more, a dst whose extent overlaps src's, and with
 * extrapolate a NULL workspace or one that overlaps src or dst. */
int nconv_depth_ipbasic(const struct nconv_depth_ipbasic* d, float* dst, long long dst_image_stride,
                        long long dst_row_stride, float* work_plane, int* work_top, void* stream);

/* Added under ABI 27 (purely additive: one new entry point and one new struct, nothing existing
 * changes, so NCONV_ABI_VERSION stays 27). The nearest-sample transform of a sparse depth plane: for
 * every pixel which input sample is nearest and how far away it is, the exact Euclidean distance
 * transform with its feature map. Nearest-neighbour interpolation (the other non-learned baseline of the
 * depth-completion tables; it fills every pixel and keeps its input samples bit for bit), the distance
 * to the nearest sample as a plane (an input channel, a confidence prior, the strata of a
 * distance-stratified error), and the mask "farther than r pixels from any return". Integer geometry:
 * no floating-point arithmetic takes part in any decision. For image b of the (B, H, W) view and pixel
 * p = (r, c):
 *   validity    a pixel q = (r', c') is a sample iff its value is finite and > floor. floor = -inf makes
 *               every finite value a sample; NaN, +-inf, and -0.0 / +0.0 under floor = 0 are not samples.
 *   distance    d2(p, q) = (r - r')^2 + (c - c')^2, an int32: shapes with H^2 + W^2 >= 2^31 are refused.
 *   nearest     near(p) = the sample of the same image with the smallest d2, ties to the smallest pixel
 *               number r' * W + c'. A sample is its own nearest (d2 = 0).
 *   range       with max_dist2 >= 0, a pixel whose nearest sample has d2 > max_dist2 has none;
 *               max_dist2 < 0: no limit. An image without samples has none anywhere.
 *   outputs     each optional (NULL: skipped), at least one required:
 *               dst    fp32 view with its own strides: the source value at near(p), bit for bit;
 *                      +0.0f where there is none
 *               index  (B, H, W) int32 contiguous: the pixel number of near(p); -1
 *               dist2  (B, H, W) int32 contiguous: d2(p, near(p)); 0x7FFFFFFF (so that the mask
 *                      dist2 <= r^2 is false there)
 *               dist   (B, H, W) fp32 contiguous: the correctly rounded sqrtf((float)d2); +inf
 * The result is a function of the input alone: identical on every run. The source is only read.
 * (the struct tag shares its name with the entry point: spell the type `struct nconv_depth_nearest`
 * or nconv_depth_nearest_desc) */
typedef struct nconv_depth_nearest {
    int B, H, W;
    const float* src;               /* fp32 view: B planes of H rows of W, 4-byte aligned          */
    long long src_image_stride;     /* elements; ignored when B == 1                               */
    long long src_row_stride;       /* elements, >= W                                              */
    float floor;                    /* a sample is finite and > floor; -inf: every finite value    */
    int max_dist2;                  /* >= 0: the largest d2 that counts; < 0: no limit             */
} nconv_depth_nearest_desc;

/* dst: fp32 view of B planes of H rows of W with its own strides in elements; index, dist2, dist:
 * contiguous (B, H, W) planes; whichever is not NULL is overwritten entirely. work: a contiguous
 * (B, H, W) int32 plane, required and overwritten (per pixel the row of the nearest sample of its
 * column, the upper one on a tie, -1 for a column without samples). src, work and the outputs must be
 * pairwise disjoint: other pixels are read, so there is no in-place operation, and the host compares
 * the byte extents.
 * Two kernels on `stream`: a column pass into work (a wave takes 64 rows of 64 columns, their validity
 * as one 64-bit mask per lane) and a row pass that searches outwards from the pixel's own column for
 * the smallest key (d2 << 32) | pixel number until the squared column offset exceeds the best d2 or
 * max_dist2, O(distance to the nearest sample) per pixel and O(W) at worst. No atomics, no host
 * synchronisation, no allocation, no waiting between workgroups: capturable. No byte outside the source
 * view's extent is read.
 * -EINVAL before any launch for a NULL descriptor / src / work, all four outputs NULL, B, H or W <= 0,
 * B * H * W >= 2^31, H^2 + W^2 >= 2^31, a NaN floor, a pointer that is not 4-byte aligned, a src or dst
 * view whose strides are smaller than its rows / images or whose image spans 2^31 bytes or more, and
 * src, work or an output overlapping another of them. */
int nconv_depth_nearest(const struct nconv_depth_nearest* d, float* dst, long long dst_image_stride,
                        long long dst_row_stride, int* index, int* dist2, float* dist, int* work, void* stream);

/* Depth-driven view warp and photometric loss (new entry points only: no existing struct or signature
 * changes, so NCONV_ABI_VERSION stays 27). The self-supervised term of Ma, Cavalheiro and Karaman (ICRA
 * 2019, "Self-supervised Sparse-to-Dense") and the monodepth family: the predicted depth of the current
 * (target) view and a known relative pose warp a neighbouring (source) camera frame into the target view,
 * and the difference to the target frame is penalised, the gradient flowing into the depth. The geometry
 * is nconv_backproject's point followed by nconv_lidar_project's projection; what is new is the bilinear
 * sampling and its derivative. Each target pixel owns its four taps, so the gradient with respect to the
 * depth is a gather: no atomics, the same bits on every run.
 *
 * The rule, fp32, one rounding per operation in the order written, no contraction. Per target pixel
 * (b, i, j) with z = depth[b][i][j]; fx, fy, cx, cy = K[0][0], K[1][1], K[0][2], K[1][2] of image b's
 * 3 x 3 matrix k (k_image_stride 0: one camera); m the row-major 3 x 4 matrix of image b
 * (m_image_stride 0: one matrix), K_src . [R | t], which takes the target camera frame to source pixels:
 *     point       tx = (float)j - cx            ty = (float)i - cy
 *                 x  = (tx * z) / fx            y  = (ty * z) / fy        (nconv_backproject's point)
 *                 pvalid = z > z_min && z <= z_max      (z_max == 0: FLT_MAX; comparisons: a NaN is not valid)
 *     project     dot(r, P) = ((r[0] * x + r[1] * y) + r[2] * z) + r[3]    (nconv_lidar_project's dot)
 *                 a = dot(m[0], P)   bb = dot(m[1], P)   c = dot(m[2], P)
 *                 u = a / c          v = bb / c                             (IEEE division)
 *     valid       pvalid && c > 0 && u >= 0 && u <= (float)(Ws - 1) && v >= 0 && v <= (float)(Hs - 1)
 *                 && (mask == NULL || mask[b][i][j] != 0)
 *                 all float comparisons made before any integer conversion
 *     taps        fu = floorf(u)     j0 = (int)fu   j1 = min(j0 + 1, Ws - 1)   wu = u - fu   w0u = 1.0f - wu
 *                 fv = floorf(v)     i0 = (int)fv   i1 = min(i0 + 1, Hs - 1)   wv = v - fv   w0v = 1.0f - wv
 *     per channel ch, a00 = src[b][ch][i0][j0], a01 = [i0][j1], a10 = [i1][j0], a11 = [i1][j1]:
 *                 top = (w0u * a00) + (wu * a01)
 *                 bot = (w0u * a10) + (wu * a11)
 *                 s   = (w0v * top) + (wv * bot)
 *                 warped[b][ch][i][j] = valid ? s : +0.0f
 *     derivatives dIu = (w0v * (a01 - a00)) + (wv * (a11 - a10))          dIv = bot - top
 *                 X   = tx / fx                  Y   = ty / fy
 *                 a'  = ((m[0][0] * X) + (m[0][1] * Y)) + m[0][2]          likewise b' (row 1) and c' (row 2)
 *                 du  = (a' - (u * c')) / c      dv  = (b' - (v * c')) / c
 *                 t[ch]   = g_s[ch] * ((dIu[ch] * du) + (dIv[ch] * dv))
 *                 g_depth = valid ? (C == 1 ? t[0] : (t[0] + t[1]) + t[2]) : +0.0f
 *     nconv_view_warp_bwd takes g_s[ch] = g_warped[b][ch][i][j].
 * The photometric loss on top of the warp, with the target frame tgt (B, C, H, W):
 *     e[ch] = |s[ch] - tgt[b][ch][i][j]|
 *     term  = valid ? (C == 1 ? e[0] : (e[0] + e[1]) + e[2]) : 0
 *     n_v   = the number of valid pixels, an integer counted on the device
 *     den   = (float)C * (float)max(n_v, 1)
 *     L     = (sum term) / den
 *     kk    = gloss * (1.0f / den)            (gloss NULL: 1)
 *     g_s[ch] = kk * sign(s[ch] - tgt[b][ch][i][j]),  sign(d) = d > 0 ? 1 : d < 0 ? -1 : 0
 *     and g_depth as above; neither warped nor g_s reaches memory.
 * The sum: fp32 partials over fixed 16 x 64 tiles (1024 terms each), tiles and images combined in double
 * in a fixed order, divided by den in double and rounded to fp32 once; the count is exact; no atomics.
 * nconv_photo_loss_fwd leaves L in loss[0] and n_v in the first int of the workspace (both on the device);
 * nconv_photo_loss_bwd reads n_v from the same workspace: no host synchronisation.
 *
 * NOT offered: a gradient with respect to the source image (a scatter); a gradient with respect to m
 * (poses are inputs); an image pyramid (a caller downsamples and scales k and m themselves). (The SSIM term is
 * nconv_photo_ssim_loss_* below; the pose itself comes from nconv_pose_normal_eq / nconv_pose_update.) An invalid pixel loads no tap, a valid one reads taps inside the source plane by the
 * clamps: no byte outside a view's extent is read.
 * (the entry points are nconv_view_warp_fwd / _bwd; the descriptor's type is `struct nconv_view_warp`
 * or nconv_view_warp_desc) */
typedef struct nconv_view_warp {
    int B, C;                       /* C = 1 or 3 channels of src (and tgt)                        */
    int H, W;                       /* the target view: depth, mask, tgt, warped, valid, g_depth   */
    int Hs, Ws;                     /* the source frame                                            */
    const float* depth;             /* fp32 view: B planes of H rows of W, 4-byte aligned          */
    long long depth_image_stride;   /* elements; ignored when B == 1                               */
    long long depth_row_stride;     /* elements, >= W                                              */
    const unsigned char* mask;      /* uint8 view (B, H, W), or NULL: every pixel may be valid     */
    long long mask_image_stride;    /* bytes; ignored when B == 1                                  */
    long long mask_row_stride;      /* bytes, >= W                                                 */
    const float* src;               /* fp32 view: B images of C planes of Hs rows of Ws            */
    long long src_image_stride;     /* elements; ignored when B == 1                               */
    long long src_channel_stride;   /* elements; ignored when C == 1                               */
    long long src_row_stride;       /* elements, >= Ws                                             */
    const float* k;                 /* device: 3 x 3 row-major intrinsics of the target camera     */
    long long k_image_stride;       /* floats between the matrices of two images; 0: one camera    */
    const float* m;                 /* device: 3 x 4 row-major K_src . [R | t]                     */
    long long m_image_stride;       /* floats between the matrices of two images; 0: one matrix    */
    float z_min, z_max;             /* valid depth: z > z_min && z <= z_max; z_max == 0: FLT_MAX   */
} nconv_view_warp_desc;

/* warped: (B, C, H, W) fp32 contiguous; valid: (B, H, W) uint8 contiguous, 1 / 0; either may be NULL
 * (skipped), not both. One launch on `stream`. */
int nconv_view_warp_fwd(const struct nconv_view_warp* d, float* warped, unsigned char* valid, void* stream);
/* g_warped: (B, C, H, W) fp32 contiguous; g_depth: (B, H, W) fp32 contiguous, OVERWRITTEN. One launch. */
int nconv_view_warp_bwd(const struct nconv_view_warp* d, const float* g_warped, float* g_depth, void* stream);

/* The fused loss. tgt: fp32 view of B images of C planes of H rows of W with its own strides in
 * elements. workspace: nconv_photo_loss_workspace_bytes(B, H, W) bytes, 8-byte aligned (0: B, H or W
 * <= 0 or B * H * W >= 2^31); the forward writes it, the backward reads its first int (n_v). loss, gloss:
 * device scalars (gloss NULL: 1). g_depth: (B, H, W) fp32 contiguous, OVERWRITTEN. Two launches forward,
 * one backward; no host synchronisation, no allocation: capturable.
 * -EINVAL before any launch, for all four entry points: a NULL descriptor, depth, src, k or m; C outside
 * {1, 3}; B, H, W, Hs or Ws <= 0; H, W, Hs or Ws above 2^24 (pixel coordinates are exact floats);
 * B * C * H * W >= 2^31; a negative k or m image stride; z_min < 0 or NaN, z_max < z_min or NaN; a
 * pointer that is not aligned to its element; a view whose strides are negative or smaller than its
 * rows / planes / images, or one plane of which spans 2^31 bytes or more ("plane too large"); no output
 * at all; a NULL tgt, loss or g_depth; a workspace that is NULL, too small or not 8-byte aligned. */
size_t nconv_photo_loss_workspace_bytes(int B, int H, int W);
int nconv_photo_loss_fwd(const struct nconv_view_warp* d, const float* tgt, long long tgt_image_stride,
                         long long tgt_channel_stride, long long tgt_row_stride, float* loss, void* workspace,
                         size_t workspace_bytes, void* stream);
int nconv_photo_loss_bwd(const struct nconv_view_warp* d, const float* tgt, long long tgt_image_stride,
                         long long tgt_channel_stride, long long tgt_row_stride, const float* gloss,
                         const void* workspace, size_t workspace_bytes, float* g_depth, void* stream);

/* The photometric loss with its structural term (new entry points only: no existing struct or signature
 * changes, so NCONV_ABI_VERSION stays 27): L = alpha Lw + (1 - alpha) Lv, the loss monodepth, monodepth2 and Ma
 * et al.'s follow-ups train with (alpha = 0.85), Lv the L1 term above and Lw the mean of (1 - SSIM) / 2 over
 * 3 x 3 windows of the warped and the target frame. The descriptor, valid(p), s[ch] and the taps are exactly
 * nconv_view_warp's. The derivative of a window's SSIM with respect to a warped pixel q of it is affine in
 * (x_q, y_q), so a pixel's gradient is a sum of three coefficients over the up to nine windows that hold it
 * and the depth's gradient stays a gather: no atomics, the same bits on every run.
 *
 * The rule, fp32, one rounding per operation in the order written, no contraction. Per channel ch,
 * x = s[ch] (the warped value of a valid pixel) and y = tgt[b][ch].
 *   window     a pixel p = (b, i, j) has a window iff 1 <= i <= H - 2, 1 <= j <= W - 2 and all nine pixels of its
 *              3 x 3 neighbourhood are valid; a pixel outside the image counts as not valid. This DIFFERS from
 *              monodepth's ReflectionPad2d(1) on purpose, by a one-pixel frame: "a term counts where all its
 *              pixels count", the smoothness loss's convention, which keeps the backward a plain box sum.
 *              n_w = the number of pixels with a window, n_v = the number of valid pixels, integers counted on
 *              the device.
 *   sums       over the window's nine pixels in raster order (row i - 1 first, columns j - 1, j, j + 1),
 *              sequential, the first element taken as it is:
 *              Sx = sum x    Sy = sum y    Sxx = sum (x * x)    Syy = sum (y * y)    Sxy = sum (x * y)
 *   moments    mux = Sx / 9.0f                    muy = Sy / 9.0f
 *              vx  = (Sxx / 9.0f) - (mux * mux)   vy  = (Syy / 9.0f) - (muy * muy)
 *              vxy = (Sxy / 9.0f) - (mux * muy)                                  (monodepth's formulation)
 *   SSIM       A1 = (2.0f * (mux * muy)) + c1               A2 = (2.0f * vxy) + c2
 *              B1 = ((mux * mux) + (muy * muy)) + c1        B2 = (vx + vy) + c2
 *              D  = B1 * B2         ssim = (A1 * A2) / D                        (IEEE division)
 *              t  = (1.0f - ssim) * 0.5f
 *              e[ch] = t < 0 ? 0 : t > 1 ? 1 : t            (a NaN stays NaN)
 *              pass  = t >= 0 && t <= 1                     (where torch.clamp passes the gradient)
 *              x == y gives ssim == 1.0f exactly (the products by 2 are exact, so A1 == B1 and A2 == B2).
 *   constants  c1 = (0.01 R)^2, c2 = (0.03 R)^2 for the data range R (255 for 8-bit-valued frames, 1 for
 *              [0, 1]), formed in double by the caller, rounded once to fp32 and passed as floats.
 *   loss       termw = window ? (C == 1 ? e[0] : (e[0] + e[1]) + e[2]) : 0
 *              Lw = (float)(sum termw / ((double)C * (double)max(n_w, 1)))
 *              Lv = nconv_photo_loss_fwd's L: the same terms, the same fp32 tile partials, the same tree
 *              L  = (alpha * Lw) + ((1.0f - alpha) * Lv)
 *              The SSIM terms are a second fp32 partial over the same 16 x 64 tiles (a term belongs to the
 *              window's centre), in the same lane and wave order; tiles and images combined in double in the
 *              same fixed order, as the smoothness loss's two sums are.
 *   backward   d ssim_p / d x_q = a_p + b_p x_q + c_p y_q for a pixel q of the window p, with
 *              c_p = (2.0f * A1) / (9.0f * D)
 *              b_p = -((2.0f * ssim) / (9.0f * B2))
 *              sm  = ssim * mux
 *              a_p = (2.0f * ((((muy * (A2 - A1)) / D) - (sm / B1)) + (sm / B2))) / 9.0f
 *              SA(q), SB(q), SC(q) = the sums of a, b, c over the nine window positions centred at
 *              (i - 1 .. i + 1, j - 1 .. j + 1) in raster order, sequential from +0.0f; a position that is
 *              no window or does not pass contributes +0.0f
 *              den_v = (float)C * (float)max(n_v, 1)         den_w = (float)C * (float)max(n_w, 1)
 *              kl = (gloss * (1.0f - alpha)) * (1.0f / den_v)             (gloss NULL: 1)
 *              kq = (alpha * 0.5f) * (gloss * (1.0f / den_w))
 *              g_x(q)  = -(kq * ((SA + (SB * x_q)) + (SC * y_q)))
 *              g_s[ch] = (kl * sign(x_q - y_q)) + g_x(q)
 *              and g_depth from g_s as nconv_view_warp's derivatives state.
 * REQUIRED PROPERTY: at alpha = 0 (and finite sums), L and g_depth equal nconv_photo_loss_*'s on the same
 * operands (g_x is a zero, kl is kk). nconv_photo_ssim_loss_fwd leaves L in loss[0] and n_v, n_w in the first
 * two ints of the workspace; the backward reads them there: no host synchronisation, and it recomputes the
 * warp of the tile and its halo from the depth: the forward saves no planes, and nothing per-pixel except
 * g_depth reaches memory.
 *
 * NOT offered: reflection padding; windows other than 3 x 3 (no Gaussian window); a gradient to the images.
 * (A per-pixel error map, the minimum reprojection over several sources and auto-masking are
 * nconv_photo_min_loss_* below.) Whether the SSIM
 * term improves the error on KITTI with this network has not been measured by anyone.
 *
 * workspace: nconv_photo_ssim_workspace_bytes(B, H, W) bytes, 8-byte aligned (0: B, H or W <= 0 or B * H * W
 * >= 2^31). tgt, loss, gloss and g_depth as nconv_photo_loss_*'s. Two launches forward, one backward; no
 * atomics, no host synchronisation, no allocation: capturable.
 * -EINVAL before any launch: everything nconv_photo_loss_* refuses; alpha outside [0, 1] or NaN; c1 or c2
 * not finite or not > 0; a workspace that is NULL, too small or not 8-byte aligned. */
size_t nconv_photo_ssim_workspace_bytes(int B, int H, int W);
int nconv_photo_ssim_loss_fwd(const struct nconv_view_warp* d, const float* tgt, long long tgt_image_stride,
                              long long tgt_channel_stride, long long tgt_row_stride, float alpha, float c1, float c2,
                              float* loss, void* workspace, size_t workspace_bytes, void* stream);
int nconv_photo_ssim_loss_bwd(const struct nconv_view_warp* d, const float* tgt, long long tgt_image_stride,
                              long long tgt_channel_stride, long long tgt_row_stride, float alpha, float c1, float c2,
                              const float* gloss, const void* workspace, size_t workspace_bytes, float* g_depth,
                              void* stream);

/* The minimum reprojection over several sources, with auto-masking (new entry points only: no existing struct
 * or signature changes, so NCONV_ABI_VERSION stays 27): monodepth2's per-pixel minimum of the photometric error
 * over the previous and the next frame, which Ma et al.'s self-supervised sparse-to-dense also warps from. A
 * pixel that one neighbouring frame sees occluded, or that left it, takes its error from the frame that does
 * see it; with auto-masking a pixel whose UNWARPED neighbour already matches the target at least as well (a
 * standing camera, an object moving with it) adds nothing. The pose side needs nothing new:
 * nconv_pose_normal_eq / nconv_pose_update are called once per source.
 *
 * The rule, fp32, one rounding per operation in the order written, no contraction. Everything not restated
 * here is nconv_view_warp's and nconv_photo_ssim_loss_*'s rule, bit for bit: valid, the taps, s[ch], the
 * derivatives, window, the nine-pixel sums, ssim, e[ch], pass, the coefficients a_p, b_p, c_p, c1, c2.
 *   sources    S sources, 1 <= S <= 4, each with its own src view (of its own size Hs x Ws) and its own m.
 *              They share depth, mask, k, tgt, z_min, z_max, B, C, H, W. valid_s, window_s, x_s = s_s[ch] are
 *              those of source s. Per target pixel p and source s:
 *              tl_s(p) = nconv_photo_loss_fwd's term, the channel sum of |x - y|
 *              tw_s(p) = termw of the SSIM rule, the channel sum of e[ch]
 *              comparable_s(p) = alpha == 0 ? valid_s(p) : window_s(p)
 *              E_s(p) = (alpha * tw_s) + ((1.0f - alpha) * tl_s); at alpha == 0 no window quantity is formed
 *              and E_s = tl_s
 *   minimum    best undefined, winner none; for s = 0 .. S - 1 in order, over the comparable sources, source s
 *              replaces the winner iff winner is none, or E_s < best, or E_s is NaN and best is not. The
 *              lowest index wins a tie (DETERMINISTIC, where monodepth2 breaks ties by random noise), and a
 *              NaN stays, as torch.min propagates it. n_c = the number of pixels that have a winner.
 *   auto-mask  optional; needs Hs == H && Ws == W for every source. I_s(p) is E_s with x replaced by
 *              src_s[b][ch][i][j] and every pixel of the image taken as valid: defined for every p at
 *              alpha == 0, and off the image's one-pixel frame otherwise. Imin = the minimum of I_s over ALL S
 *              sources under the same replacement rule. A pixel with a winner is masked iff Imin <= best (the
 *              identity wins ties, so two equal frames train nothing; a NaN on either side: not masked).
 *              n_m = the number of masked pixels; a pixel is kept iff it has a winner and is not masked.
 *   loss       L = (float)(sum over kept pixels of best / ((double)C * (double)max(n_c, 1)))
 *              fp32 partials over the same fixed 16 x 64 tiles, in the same lane, wave, tile and image order as
 *              nconv_photo_loss_fwd (a pixel that is not kept adds +0.0f). The denominator is n_c, NOT the
 *              kept count: a masked pixel adds nothing to the sum but stays in the mean, which is monodepth2's
 *              gradient scale and does not jump when the mask flickers. The VALUE differs from monodepth2's,
 *              which also adds the identity error of the masked pixels as a constant.
 *   outputs    winner (optional): uint8 (B, H, W), s, 254 for masked, 255 for none
 *              error (optional): fp32 (B, H, W), kept ? best / (float)C : +0.0f, the per-pixel error map
 *   backward   den = (float)C * (float)max(n_c, 1)
 *              kl = (gloss * (1.0f - alpha)) * (1.0f / den)               (gloss NULL: 1)
 *              kq = (alpha * 0.5f) * (gloss * (1.0f / den))
 *              for source s and pixel q, SA_s, SB_s, SC_s = the SSIM rule's nine-position sums, in which a
 *              position p' contributes only if p' is kept, winner(p') == s and the channel passes; otherwise
 *              it contributes +0.0f
 *              g_x,s(q)  = -(kq * ((SA_s + (SB_s * x_s,q)) + (SC_s * y_q)));  at alpha == 0 no window quantity
 *                          is formed and g_x,s = +0.0f
 *              g_s,ch(q) = ((q kept && winner(q) == s) ? kl * sign(x_s,q - y_q) : +0.0f) + g_x,s(q)
 *              t_s = valid_s(q) ? nconv_view_warp's channel sum of g_s,ch * ((dIu * du) + (dIv * dv)), with
 *                    source s's own du, dv : +0.0f
 *              g_depth(q) = t_0 taken as it is, then + t_1, + t_2, + t_3 in that order
 *              A pixel that lost to another source still receives the SSIM gradient of neighbouring windows
 *              that source s won. Every sum is a gather: no atomics, the same bits on every run.
 * REQUIRED PROPERTIES (finite sums): S = 1 without auto-masking gives, at alpha = 0, L and g_depth equal to
 * nconv_photo_loss_*'s and, at alpha = 1, equal to nconv_photo_ssim_loss_*'s at alpha = 1. For 0 < alpha < 1
 * this is a DIFFERENT loss from nconv_photo_ssim_loss_*: one mean over the comparable pixels (those with a
 * window) instead of two means over n_w and n_v; no equality is claimed there.
 * Deviations from monodepth2, all on purpose: the one-pixel frame and the all-valid window (no reflection
 * padding); the denominator n_c; the deterministic tie rule in place of random noise; no identity constant in
 * the value. Nobody has measured whether minimum reprojection or auto-masking improves the error on KITTI
 * with this network, and the data loaders hand out no neighbouring frames.
 *
 * NOT offered: more than four sources; a per-source weight; a gradient to the images or to m; reflection
 * padding; an image pyramid (as nconv_view_warp's).
 *
 * views: a HOST array of S descriptors. tgt, loss, gloss and g_depth as nconv_photo_loss_*'s. automask: 0 or 1.
 * workspace: nconv_photo_min_workspace_bytes(B, H, W) bytes, 8-byte aligned (0: B, H or W <= 0 or B * H * W
 * >= 2^31); the forward writes it (its first two ints are n_c, n_m; it holds the winner byte plane), the
 * backward reads it. winner, error: contiguous, either may be NULL. Two launches forward, one backward,
 * whatever S; no atomics, no host synchronisation, no allocation: capturable.
 * -EINVAL before any launch: everything nconv_photo_ssim_loss_* refuses, for each view ("view s: ..."); S
 * outside 1..4; views that disagree in B, C, H, W, the depth view, the mask view, k, z_min or z_max; automask
 * outside {0, 1}, or 1 with a source whose size is not (H, W); a workspace that is NULL, too small or not
 * 8-byte aligned; a NULL loss or g_depth. */
size_t nconv_photo_min_workspace_bytes(int B, int H, int W);
int nconv_photo_min_loss_fwd(const struct nconv_view_warp* views, int S, const float* tgt,
                             long long tgt_image_stride, long long tgt_channel_stride, long long tgt_row_stride,
                             float alpha, float c1, float c2, int automask, float* loss, unsigned char* winner,
                             float* error, void* workspace, size_t workspace_bytes, void* stream);
int nconv_photo_min_loss_bwd(const struct nconv_view_warp* views, int S, const float* tgt,
                             long long tgt_image_stride, long long tgt_channel_stride, long long tgt_row_stride,
                             float alpha, float c1, float c2, int automask, const float* gloss,
                             const void* workspace, size_t workspace_bytes, float* g_depth, void* stream);

/* Cross-view depth consistency: the check with fusion, and the geometry-consistency loss (new entry points
 * only: no existing struct or signature changes, so NCONV_ABI_VERSION stays 27). Everything above uses a
 * neighbouring frame through its colours; these compare the DEPTH of two views. nconv_depth_consistency is the
 * geometric check of MVSNet's filter_depth and COLMAP's fusion: project a target pixel into the neighbour, read
 * the neighbour's depth there, carry that point back, and keep the pixel only if it lands where it started, at
 * the depth it started with; the kept pixels' depths are averaged over the views that agree.
 * nconv_geo_consistency_loss_* is the geometry-consistency term of SC-SfMLearner (Bian et al., NeurIPS 2019),
 * which ties the scale of consecutive predictions together and whose per-pixel map is the usual occlusion /
 * moving-object mask of the photometric losses.
 *
 * The rule, fp32, one rounding per operation in the order written, no contraction. For each target pixel
 * (b, i, j) with z = depth[b][i][j], and each source s = 0 .. S - 1 in order (1 <= S <= 4):
 *   descriptor  source s is a struct nconv_view_warp whose src is the source view's DEPTH plane (C == 1), k the
 *               target intrinsics and m = K_s . [R | t]; the S descriptors share B, H, W, the depth view, the
 *               mask view, k, z_min and z_max. A struct nconv_consistency_source adds two device matrices, each
 *               with an image stride (0: shared by the batch): k_src, 3 x 3 row-major, of which
 *               fxs, fys, cxs, cys = [0][0], [1][1], [0][2], [1][2] are read as k's are; m_back, 3 x 4 row-major,
 *               K_tgt . [R | t]^-1, which takes the source camera frame to target pixels.
 *   projection  pvalid, valid, u, v, c, the taps a00 .. a11, the weights and the blend s (here zs) are
 *               nconv_view_warp's, bit for bit, the optional target mask and z_min / z_max included.
 *   tvalid      every one of the four taps t satisfies t > z_min && t <= z_max (written this way so that a NaN
 *               or the 0 of a hole of a sparse plane is not valid): a blend is never taken across an invalid tap
 *   point       xs = ((u - cxs) * zs) / fxs          ys = ((v - cys) * zs) / fys
 *   way back    a2 = dot(m_back[0], (xs, ys, zs))    likewise b2 (row 1) and c2 (row 2)   (nconv_lidar_project's dot)
 *               u2 = a2 / c2       v2 = b2 / c2       z2 = c2
 *   errors      du = u2 - (float)j                   dv = v2 - (float)i
 *               d2 = (du * du) + (dv * dv)           rz = fabsf(z2 - z)           tol2 = px_tol * px_tol
 *   decision    cons_s = valid && tvalid && c2 > 0 && d2 <= tol2 && rz <= rel_tol * z
 *               float comparisons: a NaN is not consistent
 *   fusion      n = the number of consistent sources; acc = z, then acc = acc + z2_s for the consistent
 *               sources in index order; fused = (pvalid && n >= min_views) ? acc / (float)(n + 1) : +0.0f
 *               (0 <= min_views <= S; at min_views == 0 a valid pixel without a consistent source keeps z)
 *   outputs     fused (B, H, W) fp32; count (B, H, W) uint8 = n; views (B, H, W) uint8, bit s = cons_s;
 *               reproj and reldiff (B, S, H, W) fp32 = d2 and rz / z, +inf where !(valid && tvalid && c2 > 0),
 *               so that a threshold on them is false there. Each may be NULL (skipped), not all.
 * The loss takes ONE source and nothing from m_back or k_src. On the pixels with valid && tvalid (counted):
 *               num = c - zs          den = c + zs          diff = fabsf(num) / den
 *               L = (sum diff) / max(n_g, 1),   n_g the counted pixels, an integer counted on the device
 *   c is the point's depth in the source camera only when the third row of K_src is (0 0 1); the loaders'
 *   matrices satisfy this, and it is NOT checked on the device.
 *   backward    sg  = num > 0 ? 1 : num < 0 ? -1 : 0
 *               dc  = c' of nconv_view_warp's derivatives
 *               dzs = (dIu * du) + (dIv * dv), nconv_view_warp's dIu, dIv, du, dv taken on the depth taps
 *               kk  = gloss * (1.0f / (float)max(n_g, 1))                               (gloss NULL: 1)
 *               g_depth = (kk * sg) * ((((dc - dzs) * den) - (num * (dc + dzs))) / (den * den)),
 *               +0.0f off the counted pixels. A gather: no atomics, the same bits on every run.
 * The sum is nconv_photo_loss_fwd's tree: fp32 partials over fixed 16 x 64 tiles, tiles and images combined in
 * double in a fixed order, divided by max(n_g, 1) in double and rounded to fp32 once; the count is exact and
 * left in the first int of the workspace for the backward: no host synchronisation.
 *
 * NOT offered: a gradient with respect to the source depth (a scatter) or to the pose; confidence-weighted
 * averaging; per-image kept counts; more than four sources. The symmetric loss of the paper is two calls with
 * the roles and the pose swapped. The defaults callers use (px_tol 1, rel_tol 0.01, min_views 1) are MVSNet's
 * convention; nobody has measured them on KITTI with this network. An invalid pixel loads no tap, a valid one
 * reads taps inside the source plane by the clamps: no byte outside a view's extent is read.
 *
 * views, sources: HOST arrays of S entries. fused, count, views_out, reproj, reldiff: contiguous. One launch
 * whatever S. loss, gloss: device scalars; diff: (B, H, W) fp32 contiguous, the per-pixel term, +0.0f where not
 * counted, or NULL; g_depth: (B, H, W) fp32 contiguous, OVERWRITTEN. workspace:
 * nconv_geo_consistency_workspace_bytes(B, H, W) bytes, 8-byte aligned (0: B, H or W <= 0 or B * H * W >= 2^31).
 * Two launches forward, one backward; no atomics, no host synchronisation, no allocation: capturable.
 * -EINVAL before any launch: everything nconv_view_warp_* refuses, for each view ("view s: ..."); C != 1; S
 * outside 1..4; a NULL k_src or m_back, or a negative image stride of either; views that disagree in what they
 * share; px_tol or rel_tol negative or NaN; min_views outside 0..S; no output at all; B * S * H * W >= 2^31; for
 * the loss a NULL loss or g_depth, and a workspace that is NULL, too small or not 8-byte aligned. */
typedef struct nconv_consistency_source {
    const float* k_src;             /* device: 3 x 3 row-major intrinsics of the source camera     */
    long long k_src_image_stride;   /* floats between the matrices of two images; 0: one camera    */
    const float* m_back;            /* device: 3 x 4 row-major K_tgt . [R | t]^-1                  */
    long long m_back_image_stride;  /* floats between the matrices of two images; 0: one matrix    */
} nconv_consistency_source_desc;

int nconv_depth_consistency(const struct nconv_view_warp* views, const struct nconv_consistency_source* sources,
                            int S, float px_tol, float rel_tol, int min_views, float* fused, unsigned char* count,
                            unsigned char* views_out, float* reproj, float* reldiff, void* stream);
size_t nconv_geo_consistency_workspace_bytes(int B, int H, int W);
int nconv_geo_consistency_loss_fwd(const struct nconv_view_warp* d, float* loss, float* diff, void* workspace,
                                   size_t workspace_bytes, void* stream);
int nconv_geo_consistency_loss_bwd(const struct nconv_view_warp* d, const float* gloss, const void* workspace,
                                   size_t workspace_bytes, float* g_depth, void* stream);

/* Relative camera pose from sparse depth by direct image alignment (new entry points only: no existing struct
 * or signature changes, so NCONV_ABI_VERSION stays 27). The m = K_src . [R | t] that nconv_view_warp_*,
 * nconv_photo_loss_* and nconv_photo_ssim_loss_* take as an input, estimated from what a training batch holds:
 * the sparse depth of the current (target) frame gives 3-D points, and the pose is the one that minimises the
 * intensity difference between the target frame at those pixels and the neighbouring (source) frame at their
 * projections (Kerl, Sturm, Cremers, ICRA 2013; LSD-SLAM's tracker), by damped Gauss-Newton on SE(3). One
 * iteration is nconv_pose_normal_eq followed by nconv_pose_update.
 *
 * nconv_pose_normal_eq, fp32, one rounding per operation in the order written, no contraction. Per target
 * pixel (b, i, j): P = (x, y, z), u, v, valid, the taps, s[ch], dIu[ch] and dIv[ch] are nconv_view_warp's with
 * the current m, bit for bit (a pixel is a sample iff it is valid there: z > z_min && z <= z_max, its mask, its
 * projection inside the source). With p the current fp32 pose [R | t] of image b (row-major 3 x 4) and
 * fxs = K_src[0][0], fys = K_src[1][1]:
 *     point      X' = dot(p[0], P)   Y' = dot(p[1], P)   Z' = dot(p[2], P)        (nconv_lidar_project's dot)
 *                xn = X' / Z'   yn = Y' / Z'   iz = 1.0f / Z'   xx = xn * xn   yy = yn * yn   xy = xn * yn
 *     Ju         [fxs * iz, 0, -(fxs * (xn * iz)), -(fxs * xy), fxs * (1.0f + xx), -(fxs * yn)]
 *     Jv         [0, fys * iz, -(fys * (yn * iz)), -(fys * (1.0f + yy)), fys * xy, fys * xn]
 *     J[ch]      J[0] = dIu * Ju[0]   J[1] = dIv * Jv[1]   J[k] = (dIu * Ju[k]) + (dIv * Jv[k]), k = 2 .. 5
 *                the derivative of s[ch] for a left perturbation xi = (nu, omega), dP' = nu + omega x P'
 *     residual   r = s[ch] - tgt[b][ch][i][j]      ar = |r|
 *     weight     w = (huber == 0 || ar <= huber) ? 1.0f : huber / ar                (Huber; 0: least squares)
 *     terms      wj[k] = w * J[k]   h[k][l] = wj[k] * J[l] (k <= l, row-major upper triangle: 21)
 *                bk[k] = wj[k] * r (6)   e = (w * r) * r
 *                each of the 28 summed over the channels as (t[0] + t[1]) + t[2] (C == 1: t[0]); 0 where the
 *                pixel is not valid
 * The sums are the photometric loss's: fp32 partials over fixed 16 x 64 tiles in nconv_photo_loss_fwd's lane and
 * wave order, the exact count n of valid pixels per tile; no atomics.
 *
 * nconv_pose_update, one wave per image, all of it in double (IEEE, the order written, no contraction):
 *     sums       S[0 .. 27], n: the image's tiles combined in double in nconv_photo_loss_fwd's fixed order
 *     history    cost[b][it] = (float)(S[27] / ((double)C * (double)max(n, 1)))       n_hist[b][it] = n
 *     apply == 0 stops here (the cost at the pose already reached). Otherwise:
 *     system     A = H (symmetric, from S[0 .. 20]), A[k][k] = A[k][k] + ((double)damping * A[k][k]), g = -S[21 + k]
 *     solve      A = L D L^T, the square-root-free Cholesky (only + - x /, so that a host restatement gives the
 *                same bits), for j = 0 .. 5: v[k] = L[j][k] * D[k] and d = A[j][j] - sum_{k < j} L[j][k] * v[k]
 *                (k ascending, each product subtracted in turn); D[j] = d; L[i][j] = (A[i][j] - sum_{k < j}
 *                L[i][k] * v[k]) / d for i > j. Then y[i] = g[i] - sum_{k < i} L[i][k] * y[k] and, for
 *                i = 5 .. 0, delta[i] = y[i] / D[i] - sum_{k > i} L[k][i] * delta[k] (k ascending).
 *     status     1: n < min_points; 2: a pivot d that is not finite or <= 0; 3: a delta that is not finite;
 *                0 otherwise. A nonzero status leaves the pose as it is (delta = 0).
 *     retraction (Cayley: only + - x /, unlike sin / cos) a = delta[3 .. 5] / 2, qkl = a[k] * a[l],
 *                f = 2 / (1 + ((q00 + q11) + q22)), dR = I + f ([a]x + [a]x^2):
 *                dR[0][0] = 1 + f * (-(q11 + q22))   dR[0][1] = f * (-a2 + q01)   dR[0][2] = f * (a1 + q02)
 *                dR[1][0] = f * (a2 + q01)   dR[1][1] = 1 + f * (-(q00 + q22))   dR[1][2] = f * (-a0 + q12)
 *                dR[2][0] = f * (-a1 + q02)  dR[2][1] = f * (a0 + q12)    dR[2][2] = 1 + f * (-(q00 + q11))
 *                [R | t] <- dR . [R | t] with (dR[i][0] * P[0][j] + dR[i][1] * P[1][j]) + dR[i][2] * P[2][j],
 *                then t[i] <- t[i] + delta[i]
 *     outputs    pose[b] = (float)[R | t];  m[b][i][j] = (float)((Ks[i][0] * P[0][j] + Ks[i][1] * P[1][j]) +
 *                Ks[i][2] * P[2][j]) with Ks = (double)K_src, for the next nconv_pose_normal_eq
 * The pose state is the double (B, 3, 4) at the start of the workspace, so that orthogonality does not drift with
 * the fp32 rounding of `pose`; THE CALLER INITIALISES IT (and pose and m to match) before the first iteration.
 * The B x 28 doubles after it are the sums S as the last update combined them.
 *
 * NOT offered: feature matching or PnP; RANSAC; a step-acceptance test (true Levenberg-Marquardt: the damping is
 * fixed); joint refinement of the depth; more than one source per call; affine brightness correction; an image
 * pyramid (a caller runs the levels, coarse to fine, on its own downsampled operands).
 *
 * The descriptor is nconv_view_warp's fields, then the new ones. m and pose are read by nconv_pose_normal_eq and
 * rewritten by nconv_pose_update; with B > 1 each image has its own m (m_image_stride >= 12). status: (B) int;
 * cost, n_hist: (B, history) fp32 / int rows, entry `it` written by nconv_pose_update(.., it, ..). workspace:
 * nconv_pose_workspace_bytes(B, H, W) bytes, 8-byte aligned (0: B, H or W <= 0 or B * H * W >= 2^31). One launch
 * each; no host synchronisation, no allocation: capturable.
 * -EINVAL before any launch: everything nconv_photo_loss_fwd refuses of the shared fields and tgt; a NULL k_src,
 * pose, status, cost or n_hist; a pointer that is not 4-byte aligned; a negative k_src image stride; with B > 1
 * an m_image_stride below 12; a negative or NaN huber or damping; min_points < 6; history <= 0; it outside
 * [0, history); a workspace that is NULL, too small or not 8-byte aligned. */
typedef struct nconv_pose_align {
    int B, C;                       /* C = 1 or 3 channels of src and tgt                          */
    int H, W;                       /* the target view: depth, mask, tgt                           */
    int Hs, Ws;                     /* the source frame                                            */
    const float* depth;             /* the sparse depth of the target: fp32 view, B planes of H x W */
    long long depth_image_stride;   /* elements; ignored when B == 1                               */
    long long depth_row_stride;     /* elements, >= W                                              */
    const unsigned char* mask;      /* uint8 view (B, H, W), or NULL                               */
    long long mask_image_stride;    /* bytes; ignored when B == 1                                  */
    long long mask_row_stride;      /* bytes, >= W                                                 */
    const float* src;               /* fp32 view: B images of C planes of Hs rows of Ws            */
    long long src_image_stride;     /* elements; ignored when B == 1                               */
    long long src_channel_stride;   /* elements; ignored when C == 1                               */
    long long src_row_stride;       /* elements, >= Ws                                             */
    const float* k;                 /* device: 3 x 3 row-major intrinsics of the target camera     */
    long long k_image_stride;       /* floats between the matrices of two images; 0: one camera    */
    float* m;                       /* device: 3 x 4 row-major K_src . [R | t], read and REWRITTEN */
    long long m_image_stride;       /* floats between the matrices of two images, >= 12 (B > 1)    */
    float z_min, z_max;             /* a sample: z > z_min && z <= z_max; z_max == 0: FLT_MAX      */
    const float* tgt;               /* fp32 view: B images of C planes of H rows of W              */
    long long tgt_image_stride;     /* elements; ignored when B == 1                               */
    long long tgt_channel_stride;   /* elements; ignored when C == 1                               */
    long long tgt_row_stride;       /* elements, >= W                                              */
    const float* k_src;             /* device: 3 x 3 row-major intrinsics of the source camera     */
    long long k_src_image_stride;   /* floats between the matrices of two images; 0: one camera    */
    float* pose;                    /* device: (B, 3, 4) fp32 [R | t], read and REWRITTEN          */
    int* status;                    /* device: (B) int, written by nconv_pose_update (apply != 0)  */
    float* cost;                    /* device: (B, history) fp32                                   */
    int* n_hist;                    /* device: (B, history) int                                    */
    int history;                    /* entries of a history row                                    */
    float huber;                    /* Huber threshold in units of the frames; 0: least squares    */
    float damping;                  /* A = H + damping diag(H)                                     */
    int min_points;                 /* >= 6: fewer valid pixels leave the pose as it is (status 1) */
} nconv_pose_align_desc;

size_t nconv_pose_workspace_bytes(int B, int H, int W);
int nconv_pose_normal_eq(const struct nconv_pose_align* d, void* workspace, size_t workspace_bytes, void* stream);
int nconv_pose_update(const struct nconv_pose_align* d, void* workspace, size_t workspace_bytes, int it, int apply,
                      void* stream);

/* Edge-aware depth smoothness loss and its edge weights (new entry points only: no existing struct or
 * signature changes, so NCONV_ABI_VERSION stays 27). The regulariser the photometric term above is trained
 * with: on road, sky and walls every depth explains the image equally well, so the papers pair the term with
 * a penalty on the predicted depth's differences -- the L1 of its first differences, relaxed where the image
 * itself has an edge (monodepth: Godard, Mac Aodha, Brostow, CVPR 2017; order = 1), or the L1 of its second
 * differences (Ma, Cavalheiro, Karaman, ICRA 2019; order = 2). Every pixel of the gradient gathers its own
 * stencil: no atomics, the same bits on every run.
 *
 * The rule, fp32, one rounding per operation in the order written, no contraction. Per image b: d the depth
 * view (B, H, W); M(i, j) = 0 <= i < H && 0 <= j < W && (mask == NULL || mask[b][i][j] != 0); the optional
 * weights w (B, 2, H, W) contiguous, wx(i, j) = w[b][0][i][j] the weight of the edge between columns j and
 * j + 1 (column W - 1 is never read), wy(i, j) = w[b][1][i][j] that of the edge between rows i and i + 1 (row
 * H - 1 is never read); weights == NULL: every weight is 1 and no multiply is made. min(a, b) = b < a ? b : a.
 *   order 1     x, 0 <= j <= W - 2:  cx = M(i, j) && M(i, j + 1)       tx = d[i][j + 1] - d[i][j]    ox = wx(i, j)
 *               y, 0 <= i <= H - 2:  cy = M(i, j) && M(i + 1, j)       ty = d[i + 1][j] - d[i][j]    oy = wy(i, j)
 *   order 2     x, 1 <= j <= W - 2:  cx = M(i, j - 1) && M(i, j) && M(i, j + 1)
 *                                    tx = (d[i][j - 1] + d[i][j + 1]) - (2.0f * d[i][j])
 *                                    ox = min(wx(i, j - 1), wx(i, j))
 *               y, 1 <= i <= H - 2:  likewise down the column with wy
 *   both        sx = cx ? ox * |tx| : 0                sy likewise
 *               n_x, n_y = the numbers of true cx, cy, integers counted on the device
 *               L  = (float)(Sx / (double)max(n_x, 1) + Sy / (double)max(n_y, 1)),  Sx = sum sx, Sy = sum sy
 *               kx = gloss * (1.0f / (float)max(n_x, 1))      ky likewise        (gloss NULL: 1)
 *               qx(i, j) = cx ? (kx * ox) * sign(tx) : +0.0f  qy likewise        (sign(t) = t > 0 ? 1 : t < 0 ? -1 : 0)
 *   order 1     g_depth(i, j) = ((qx(i, j - 1) - qx(i, j)) + qy(i - 1, j)) - qy(i, j)
 *   order 2     g_depth(i, j) = (((qx(i, j - 1) + qx(i, j + 1)) - (2.0f * qx(i, j)))
 *                                + (qy(i - 1, j) + qy(i + 1, j))) - (2.0f * qy(i, j))
 *               a q outside its range is +0.0f.
 * Sx and Sy are summed separately: fp32 partials over the photometric loss's fixed 16 x 64 tiles (a term
 * belongs to the pixel (i, j) it is written at), in its lane and wave order; tiles and images combined in
 * double in a fixed order; L formed in double and rounded to fp32 once. A NaN depth makes the terms it
 * touches NaN (and their q 0); a masked-out depth is never multiplied in. A 1-wide or 1-high image has
 * n_x or n_y equal to 0. nconv_smooth_loss_fwd leaves L in loss[0] and n_x, n_y in the first two ints of the
 * workspace; nconv_smooth_loss_bwd reads them there: no host synchronisation.
 *
 * The edge weights of a frame I (B, C, H, W), C = 1 or 3, alpha >= 0:
 *               e[ch] = |I[b][ch][i][j + 1] - I[b][ch][i][j]|
 *               g     = C == 1 ? e[0] : ((e[0] + e[1]) + e[2]) / 3.0f
 *               wx(i, j) = E(alpha * g);   wy(i, j) likewise from I[b][ch][i + 1][j]
 *               wx(i, W - 1) = wy(H - 1, j) = 1.0f  (written, never read by the loss)
 * E(x) stands for exp(-x), x >= 0, and is these operations (no library or hardware exponential: their
 * bits differ between hosts and the device):
 *               y = x * 1.44269504f;   y = y < 126.0f ? y : 126.0f      (a NaN or huge x ends at 126)
 *               n = rintf(y)            (to nearest, ties to even)       r = n - y   (exact, |r| <= 0.5)
 *               p = c6;  p = p * r + c5;  ..  p = p * r + c0             (Horner, product and sum rounded apiece)
 *               c0 .. c6 = 1.0f, 0.693147182f, 0.240226507f, 0.0555041097f, 0.00961812865f,
 *                          0.00133335579f, 0.000154035297f               (ln(2)^k / k!)
 *               E = n > 125.0f ? +0.0f : p * 2^-n                        (the bits (127 - (int)n) << 23: exact)
 * so weights below 2^-125.5 (x above 86.9), and those of a NaN, are +0. How far E departs from float64
 * exp(-x) is a measurement (tests/smooth_cases.py e_error: every g an 8-bit frame produces and 4097
 * significands of every binade of alpha g, g in [0, 255], where E is not flushed), largest relative error:
 *               E_MAX_REL_ERR   alpha = 1/255: 2.343e-07   alpha = 1: 3.805e-06 ;
 * the second is the rounding of x * log2(e) at y near 125.
 *
 * NOT offered: normalising the depth by its mean (or a disparity); the mixed derivative d_xy; a gradient
 * with respect to the weights or the image (both are inputs).
 * (the entry points are nconv_smooth_loss_fwd / _bwd; the descriptor's type is `struct nconv_smooth_loss`
 * or nconv_smooth_loss_desc) */
typedef struct nconv_smooth_loss {
    int B, H, W;                    /* depth, mask, g_depth: B planes of H rows of W               */
    int order;                      /* 1: first differences (monodepth); 2: second (Ma et al.)     */
    const float* depth;             /* fp32 view, 4-byte aligned                                   */
    long long depth_image_stride;   /* elements; ignored when B == 1                               */
    long long depth_row_stride;     /* elements, >= W                                              */
    const unsigned char* mask;      /* uint8 view (B, H, W), or NULL: every pixel takes part       */
    long long mask_image_stride;    /* bytes; ignored when B == 1                                  */
    long long mask_row_stride;      /* bytes, >= W                                                 */
    const float* weights;           /* fp32 (B, 2, H, W) contiguous (nconv_edge_weights), or NULL  */
} nconv_smooth_loss_desc;

/* workspace: nconv_smooth_loss_workspace_bytes(B, H, W) bytes, 8-byte aligned (0: B, H or W <= 0 or
 * B * H * W >= 2^31); the forward writes it, the backward reads its first two ints (n_x, n_y). loss, gloss:
 * device scalars (gloss NULL: 1). g_depth: (B, H, W) fp32 contiguous, OVERWRITTEN, not overlapping depth.
 * Two launches forward, one backward; no host synchronisation, no allocation: capturable.
 * -EINVAL before any launch: a NULL descriptor or depth; order outside {1, 2}; B, H or W <= 0;
 * B * H * W >= 2^31; a pointer that is not aligned to its element; a view whose strides are negative or
 * smaller than its rows / images, or one plane of which spans 2^31 bytes or more ("plane too large"); a NULL
 * loss or g_depth; g_depth overlapping depth; a workspace that is NULL, too small or not 8-byte aligned. */
size_t nconv_smooth_loss_workspace_bytes(int B, int H, int W);
int nconv_smooth_loss_fwd(const struct nconv_smooth_loss* d, float* loss, void* workspace, size_t workspace_bytes,
                          void* stream);
int nconv_smooth_loss_bwd(const struct nconv_smooth_loss* d, const float* gloss, const void* workspace,
                          size_t workspace_bytes, float* g_depth, void* stream);

/* (the entry point is nconv_edge_weights; the descriptor's type is `struct nconv_edge_weights` or
 * nconv_edge_weights_desc) */
typedef struct nconv_edge_weights {
    int B, C, H, W;                 /* C = 1 or 3 channels                                         */
    const float* image;             /* fp32 view: B images of C planes of H rows of W              */
    long long image_stride;         /* elements; ignored when B == 1                               */
    long long channel_stride;       /* elements; ignored when C == 1                               */
    long long row_stride;           /* elements, >= W                                              */
    float alpha;                    /* >= 0, finite; the monodepth recipe on 8-bit values: 1 / 255 */
} nconv_edge_weights_desc;

/* weights: (B, 2, H, W) fp32 contiguous, OVERWRITTEN, not overlapping the image. One launch on `stream`.
 * -EINVAL before any launch: a NULL descriptor, image or weights; C outside {1, 3}; B, H or W <= 0;
 * B * C * H * W >= 2^31; alpha negative, NaN or infinite; a misaligned pointer; a view refused as above;
 * weights overlapping the image. */
int nconv_edge_weights(const struct nconv_edge_weights* d, float* weights, void* stream);

/* Voxel-grid merge of point clouds (new entry points only: no existing struct or signature changes, so
 * NCONV_ABI_VERSION stays 27). The step after nconv_backproject_points, nconv_pose_* and nconv_depth_consistency:
 * the clouds of several frames, each with the pose of its camera in the world, become ONE cloud with one point
 * per occupied cell of a stated box of cubic cells: the weighted mean of the points that fell into the cell
 * (Open3D's voxel_down_sample, PCL's VoxelGrid). The rule, fp32 with one rounding per operation unless it says
 * double, no fused multiply-add anywhere:
 *
 *  rows      xyz is N rows of three fp32. With offsets (S + 1 int32, non-decreasing: the offsets of
 *            nconv_backproject_points) row i belongs to segment s iff offsets[s] <= i < offsets[s + 1]; a row
 *            below offsets[0] or at or beyond offsets[S] belongs to no segment (offsets[S] may exceed N: a
 *            truncated cloud; rows at or beyond N do not exist). The segment is found by bisection: the number
 *            of offsets <= i, minus one; with offsets that decrease somewhere a row still gets one of the S
 *            segments or none, which of them is then unspecified. Without offsets every row is in segment 0.
 *  1 world   with poses ((S, 3, 4) fp32 [R | t] of segment s, camera to world), row x = (x0, x1, x2) becomes
 *            p_k = ((R_k0 x0 + R_k1 x1) + R_k2 x2) + t_k, five roundings, the order of nconv_view_warp_*'s and
 *            nconv_lidar_project's 3 x 4 products; its normal n becomes (R_k0 n0 + R_k1 n1) + R_k2 n2. Without
 *            poses p = x and the normal stays, bit for bit (no arithmetic).
 *  2 cell    per axis a: f_a = floorf((p_a - origin_a) / voxel), one subtraction and one IEEE division. The
 *            point is INSIDE iff it belongs to a segment, its weight (weights[i], 1 without weights) is > 0, and
 *            f_a >= 0 && f_a < (float)n_a on all three axes: float comparisons before any conversion, so a NaN or
 *            an infinite coordinate is not inside. A point on the box's lower faces is inside, one on its upper
 *            faces is not. Every other row is DROPPED and counted; that includes a weight <= 0 (a negative
 *            weight cannot be refused on the host without reading device memory, so it is dropped, not an
 *            error). key = (i_z * ny + i_y) * nx + i_x with i_a = (int)f_a.
 *  3 order   the inside points are sorted by key, stably: equal keys stay in ascending input row.
 *            P = ceil(bits(nx * ny * nz - 1) / 8) radix passes of 8-bit digits, known from dims alone.
 *  4 sums    a run is a maximal stretch of equal keys in the sorted order; it becomes one output row. W = the
 *            sum of the run's weights in int64. For each of the up to nine values v of a point (p, the colour
 *            bytes as numbers, the rotated normal) the run's sum of the terms (double)w * (double)v (one
 *            rounding: the product is not exact for large weights) is taken in double in this tree: the sorted
 *            positions 0, 1, .. are cut into chunks of C = 256. The part of a run inside one chunk is a piece;
 *            a piece's sum is 0.0 + t_first + .. + t_last, left to right. The run's sum is its pieces' sums
 *            added left to right, starting from the first piece's sum. The tree depends on sorted positions
 *            only; one thread adds at most C terms and N / C pieces.
 *  5 output  row m of the outputs is the run with the m-th smallest key:
 *            xyz[m][a]     = (float)(sum of w p_a / (double)W)         (double division, then one rounding)
 *            rgb[m][a]     = (uint8)rint(sum of w c_a / (double)W)      half to even; always inside [0, 255]
 *            normals[m]    = the three sums rounded to fp32 (s_x, s_y, s_z), then l = sqrt((s_x s_x + s_y s_y) +
 *                            s_z s_z) and s / l, exactly nconv_depth_normals' last step; (0, 0, 0) unless
 *                            l > 0 && l < inf. A point whose normal is (0, 0, 0) ("none") adds zeros: it does not
 *                            move the direction.
 *            count[m]      = min(W, INT32_MAX);  key[m] = the run's key
 *            stats         = int32 {n_voxels, n_inside, n_dropped, 0}, n_inside + n_dropped = N. n_voxels is the
 *                            true number of runs even where it exceeds max_voxels; rows from
 *                            min(n_voxels, max_voxels) on are not written.
 *
 * The result is a function of the inputs alone: the same bits on every run. 5 + 2 P launches on `stream`
 * whatever the data (nx ny nz = 1: five), no global or floating-point atomics, no host synchronisation, no
 * allocation: capturable in a hipGraph. Sized for the clouds of tens of frames: every workgroup of the compaction
 * sums all N / 1024 tile counts for its base and one workgroup scans the N / 256 chunk counts, so up to N of
 * some 10^7 rows these steps are a small share; the result stays right up to the limit N < 2^31, but there
 * they take far longer than the rest. A merged map goes back in as a segment of its own with
 * weights = count to add further clouds; that is a second application of the rule (the stored means were
 * rounded to fp32), not bit-equal to one merge of everything. */
typedef struct nconv_voxel_merge_args {
    long long n_points;             /* N, 0 <= N < 2^31                                              */
    const float* xyz;               /* (N, 3) fp32 (may be NULL when N == 0)                         */
    long long xyz_row_stride;       /* elements, >= 3                                                */
    const unsigned char* rgb;       /* NULL: no colours; (N, 3) uint8                                */
    long long rgb_row_stride;       /* bytes, >= 3                                                   */
    const float* normals;           /* NULL: no normals; (N, 3) fp32, (0, 0, 0) = none               */
    long long normals_row_stride;   /* elements, >= 3                                                */
    const int* weights;             /* NULL: every weight 1; (N) int32 contiguous                    */
    const int* offsets;             /* NULL: one segment of all rows; (n_segments + 1) int32         */
    const float* poses;             /* NULL: identity; (n_segments, 3, 4) fp32 contiguous            */
    int n_segments;                 /* S >= 1; 1 without offsets                                     */
    int nx, ny, nz;                 /* cells per axis, 1 <= nx * ny * nz < 2^31                      */
    float voxel;                    /* edge of a cell, > 0 and finite                                */
    float origin[3];                /* the box's lower corner, finite                                */
    long long max_voxels;           /* rows of the outputs, 0 <= max_voxels < 2^31                   */
    float* out_xyz;                 /* (max_voxels, 3) fp32 contiguous                               */
    unsigned char* out_rgb;         /* (max_voxels, 3) uint8; required with rgb, else not written    */
    float* out_normals;             /* (max_voxels, 3) fp32; required with normals, else not written */
    int* out_count;                 /* (max_voxels) int32                                            */
    int* out_key;                   /* (max_voxels) int32                                            */
    int* stats;                     /* 4 int32                                                       */
} nconv_voxel_merge_desc;

/* workspace: nconv_voxel_merge_workspace_bytes(n_points, nx, ny, nz) bytes, 8-byte aligned, non-decreasing in
 * n_points (0: n_points < 0 or >= 2^31, a dimension <= 0, or nx * ny * nz >= 2^31). With max_voxels == 0 the
 * five out_* pointers are not read. The outputs are OVERWRITTEN and must not overlap the inputs.
 * -EINVAL before any launch: a NULL descriptor or stats; n_points or max_voxels negative or >= 2^31; NULL xyz
 * with n_points > 0; a row stride below 3 (or negative); a pointer that is not aligned to its element;
 * n_segments < 1, or != 1 without offsets; a dimension <= 0 or nx * ny * nz >= 2^31; voxel not > 0 or not
 * finite; an origin that is not finite; with max_voxels > 0 a NULL out_xyz, out_count or out_key, a NULL
 * out_rgb with rgb, a NULL out_normals with normals; a workspace that is NULL, too small or not 8-byte
 * aligned. */
size_t nconv_voxel_merge_workspace_bytes(long long n_points, int nx, int ny, int nz);
int nconv_voxel_merge(const struct nconv_voxel_merge_args* a, void* workspace, size_t workspace_bytes,
                      void* stream);

#ifdef __cplusplus
}
#endif

#endif /* NCONV_H */
