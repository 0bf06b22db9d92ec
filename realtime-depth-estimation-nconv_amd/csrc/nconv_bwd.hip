// nconv_bwd.hip — host side of the NConv backward for gfx950 (MI355X): kernel choice, workspace
// layout, validation and dispatch. Kernels and their launchers: nconv_dgrad.hip, nconv_wgrad.hip,
// nconv_wgrad_mfma.hip (exact fp32); nconv_dgrad_bf.hip, nconv_wgrad_bf.hip (split bf16).
// Autograd of NConv2d.forward (reference models/step1.py:116-149) plus its DNET glue, in closed
// form (D and N/(D+eps) recovered from the saved outputs as cout*s and y-b):
//   gN = gy/(D+eps)          gD = -gy*N/(D+eps)^2 + gcout/s
//   gb = sum gy              gs = -sum gcout*D/s^2
//   gW = corr(x*c, gN) + corr(c, gD) + gs            (weight gradient, "wgrad")
//   G  = W^T (*) {gN, gD}    gx = G_xc*c,  gc = G_c + G_xc*x     (input gradient, "dgrad")
// dgrad is the forward's packed-FP32 structure transposed: a thread owns P input pixels and
// accumulates {G_xc, G_c} += w * {gN, gD} over (o, kh, kw), with {gN, gD} computed from
// (gy, gcout, y, cout) while staging. Its epilogue routes the input gradient through the glue's
// backward: max_pool2d -> the first maximum of the window (recomputed from the producer),
// concat -> channel split, nearest upsample -> a staged plane summed by upsample_bwd_gather.
// wgrad accumulates per-workgroup partial sums in registers over several tiles and a second
// kernel reduces them in a fixed order (bitwise deterministic, no float atomics).
#include "nconv_internal.h"

namespace nconv {

static bool simple_geom(const nconv_layer& L) {
    return L.SH == 1 && L.SW == 1 && L.DH == 1 && L.DW == 1 && L.groups == 1 && L.KH == L.KW;
}

constexpr size_t kWgMaxBlocks = 4096;  // workspace bound; the launch uses at most one resident round

enum Path { kTiled, kGeneric };

static Path pick_path(const nconv_layer& L) {
    if (!simple_geom(L)) return kGeneric;
    const int m = L.load_mode;
    if ((L.Cin == 1 && L.Cout == 8 && L.KH == 5 && m == NCONV_LOAD_THRESH) ||
        (L.Cin == 8 && L.Cout == 8 && L.KH == 5 && (m == NCONV_LOAD_PLAIN || m == NCONV_LOAD_POOL2)) ||
        (L.Cin == 16 && L.Cout == 8 && L.KH == 3 && is_upcat(L)) ||
        (L.Cin == 8 && L.Cout == 1 && L.KH == 1 && m == NCONV_LOAD_PLAIN))
        return kTiled;
    return kGeneric;
}

static int generic_chunks(const nconv_layer& L) {
    const size_t np = (size_t)L.B * L.Ho * L.Wo;
    size_t c = (np + 65535) / 65536;
    if (c < 1) c = 1;
    if (c > 64) c = 64;
    return (int)c;
}

static size_t wg_blocks(const nconv_layer& L) {  // wgrad_tiled's 4 x 64 output tiles
    const size_t nt = (size_t)((L.Wo + 63) / 64) * ((L.Ho + 3) / 4) * L.B;
    return nt < kWgMaxBlocks ? nt : kWgMaxBlocks;
}

// tiled 3x3 / 5x5 layers with several input channels (Cin = 1 has a single-row A tile and stays
// on wgrad_tiled, which reads each g plane once per 4 x 64 tile instead of once per row segment)
static bool wgrad_on_mfma(const nconv_layer& L) { return L.KH > 1 && L.Cin > 1; }

// The workspace: nblk partial rows of the weight gradient (stride floats each: the weights, sum
// gy, sum gcout*cout; nblk bounds every kernel the layer's path may launch), kReduceSplit rows of
// slice sums, then from the next 256-byte boundary an UpCat layer's staged upsampled-channel planes
// tx, tc for upsample_bwd_gather (or dgrad_phase's box weights).
struct BwdLayout {
    Path path;
    size_t nblk, stride;
    size_t part_bytes;    // partial rows + slice sums, 256-rounded: the offset of tx
    size_t stage_floats;  // tx + tc (0 unless UpCat)
    size_t bytes() const { return part_bytes + stage_floats * sizeof(float); }
};

static BwdLayout bwd_layout(const nconv_layer& L) {
    BwdLayout w;
    w.path = pick_path(L);
    if (w.path == kGeneric) w.nblk = (size_t)generic_chunks(L);
    else w.nblk = wgrad_on_mfma(L) ? wgrad_mfma_max_blocks(L) : wg_blocks(L);
    w.stride = (size_t)L.Cout * (L.Cin / L.groups) * L.KH * L.KW + 2 * L.Cout;
    w.part_bytes = ((w.nblk + kReduceSplit) * w.stride * sizeof(float) + 255) & ~(size_t)255;
    const size_t planes = 2 * (size_t)L.B * L.b.C * L.H * L.W;
    w.stage_floats = is_upcat(L) ? (planes > 1024 ? planes : 1024) : 0;
    return w;
}

size_t bwd_workspace_bytes(const LayerDev& d) { return bwd_layout(d.L).bytes(); }

size_t bwd_tail_workspace_bytes(const nconv_layer& L) {
    return (wgrad_mfma_max_blocks(L) + kReduceSplit) * 10 * sizeof(float);
}

size_t bwd_head_workspace_bytes(const nconv_layer& L) {
    return (dgrad_blocks(L) + kReduceSplit) * kHeadStride * sizeof(float);
}

void plan_bwd(const nconv_layer& L, int* dgrad, int* wgrad) {
    if (pick_path(L) == kGeneric) {
        *dgrad = *wgrad = NCONV_KERNEL_GENERIC;
        return;
    }
    const int bf = L.bwd_math == NCONV_MATH_BF16X9 ? NCONV_KERNEL_MFMA_BF16X9 : NCONV_KERNEL_MFMA_BF16X3;
    const bool multi = wgrad_on_mfma(L);
    const bool fp32 = L.bwd_math == NCONV_MATH_FP32;
    *dgrad = multi && !fp32 ? bf : (dgrad_phase_ok(L) ? NCONV_KERNEL_TILED_FP32_PHASE : NCONV_KERNEL_TILED_FP32);
    *wgrad = multi ? (fp32 ? NCONV_KERNEL_MFMA_FP32 : bf) : NCONV_KERNEL_TILED_FP32;
}

// One tiled layer: the input gradient (if any is asked for), then the weight gradient's partial
// rows and their reduction. nblk_max: the rows the workspace holds (BwdLayout::nblk).
template <int CIN, int COUT, int K, int MODE, bool GP = false, bool HW = false, bool T7 = false>
static int go_bwd_tiled(const LayerDev& d, const BwdArgs& a, float* part, int nblk_max, float* tx, float* tc,
                        hipStream_t st, const char** why) {
    const nconv_layer& L = d.L;
    constexpr bool MULTI = K > 1 && CIN > 1;  // wgrad_on_mfma
    const bool fp32 = L.bwd_math == NCONV_MATH_FP32;
    const int np = L.bwd_math == NCONV_MATH_BF16X9 ? 3 : 2;  // split-bf16 parts
    if (HW || a.gxa || a.gca || a.gxb || a.gcb) {
        if constexpr (MULTI) {
            if (!fp32) go_dgrad_bf<CIN, COUT, K, MODE>(d, a, tx, tc, np, st);
        }
        if (!MULTI || fp32)
            if (int rc = go_dgrad<CIN, COUT, K, MODE, GP, HW, T7>(d, a, tx, tc, st, why)) return rc;
    }
    if (!(a.gw || a.gb)) return 0;
    int nblk;
    if constexpr (MULTI) {
        if (!fp32) {
            // (the bf16 grid cannot exceed the rows: its strips are wider than wgrad_mfma's, for which
            // the workspace is sized; checked anyway, so a bf16 request never silently runs another kernel)
            nblk = go_wgrad_bf<CIN, COUT, K, MODE>(d, a, part, nblk_max, np, st);
            if (nblk < 0) {
                *why = "bf16 weight-gradient grid exceeds the workspace";
                return -5;
            }
        } else {
            nblk = go_wgrad_mfma<CIN, COUT, K, MODE, GP, T7>(d, a, part, st);
            if constexpr (T7) {  // nconv7's weight-gradient partial rows: one per wgrad workgroup
                if (a.defer) {
                    *a.t7nparts = nblk;
                } else {
                    const RedJob J{a.t7part, a.t7s, a.t7gw, nullptr, nblk, 8, 1, 8};
                    if (int rc = launch_wgrad_reduce_multi(1, &J, st, why)) return rc;
                }
            }
        }
    } else {
        nblk = go_wgrad_tiled<CIN, COUT, K, MODE>(d, a, part, nblk_max, st);
    }
    return launch_wgrad_reduce(a, part, nblk, COUT * CIN * K * K, COUT, CIN * K * K, L.wsum, st, why);
}

int launch_bwd(const LayerDev& d, const BwdArgs& a, hipStream_t st, const char** why) {
    const nconv_layer& L = d.L;
    const BwdLayout w = bwd_layout(L);
    if (a.ws_bytes < w.bytes()) {
        *why = "workspace too small (see nconv_bwd_workspace_bytes)";
        return -22;
    }
    const Path path = w.path;
    const int nblk = (int)w.nblk;
    float* part = a.ws;
    float* tx = a.ws + w.part_bytes / sizeof(float);
    float* tc = tx + (size_t)L.B * L.b.C * L.H * L.W;

    int rc = 0;
    if (a.gpy || a.gpc || a.parg) {  // pooled-gradient routing: built for the 8->8 5x5 exact-fp32 layers
        if (!(a.gpy && a.gpc && a.parg) || path != kTiled || L.Cin != 8 || L.Cout != 8 || L.KH != 5 ||
            L.load_mode != NCONV_LOAD_PLAIN || L.bwd_math != NCONV_MATH_FP32 || L.Ho < 2 || L.Wo < 2) {
            *why = "pooled-output gradient needs gy_pool, gcout_pool and the argmax codes, on an exact-fp32 "
                   "8->8 5x5 stride-1 layer with plain loads";
            return -95;
        }
        rc = a.hpart ? go_bwd_tiled<8, 8, 5, NCONV_LOAD_PLAIN, true, true>(d, a, part, nblk, tx, tc, st, why)
                     : go_bwd_tiled<8, 8, 5, NCONV_LOAD_PLAIN, true>(d, a, part, nblk, tx, tc, st, why);
    } else if (a.t7part) {
        if (!(path == kTiled && dgrad_phase_ok(L) && L.load_mode == NCONV_LOAD_UPCAT_UP_FIRST && L.PH == 0 &&
              L.PW == 0)) {
            *why = "fused tail backward needs nconv6's exact-fp32 geometry (16->8 3x3, padding 0, upsample-first "
                   "exactly-2x concat)";
            return -95;
        }
        rc = go_bwd_tiled<16, 8, 3, NCONV_LOAD_UPCAT_UP_FIRST, false, false, true>(d, a, part, nblk, tx, tc, st, why);
    } else if (a.hpart) {
        if (!(path == kTiled && L.Cin == 8 && L.Cout == 8 && L.KH == 5 && L.load_mode == NCONV_LOAD_PLAIN &&
              L.bwd_math == NCONV_MATH_FP32)) {
            *why = "fused head weight gradient needs an exact-fp32 8->8 5x5 stride-1 layer with plain loads";
            return -95;
        }
        rc = go_bwd_tiled<8, 8, 5, NCONV_LOAD_PLAIN, false, true>(d, a, part, nblk, tx, tc, st, why);
    } else if (path == kTiled) {
        const int m = L.load_mode;
        if (L.Cin == 1 && m == NCONV_LOAD_THRESH) rc = go_bwd_tiled<1, 8, 5, NCONV_LOAD_THRESH>(d, a, part, nblk, tx, tc, st, why);
        else if (L.Cin == 8 && L.Cout == 8 && m == NCONV_LOAD_PLAIN) rc = go_bwd_tiled<8, 8, 5, NCONV_LOAD_PLAIN>(d, a, part, nblk, tx, tc, st, why);
        else if (L.Cin == 8 && L.Cout == 8 && m == NCONV_LOAD_POOL2) rc = go_bwd_tiled<8, 8, 5, NCONV_LOAD_POOL2>(d, a, part, nblk, tx, tc, st, why);
        else if (m == NCONV_LOAD_UPCAT_SKIP_FIRST) rc = go_bwd_tiled<16, 8, 3, NCONV_LOAD_UPCAT_SKIP_FIRST>(d, a, part, nblk, tx, tc, st, why);
        else if (m == NCONV_LOAD_UPCAT_UP_FIRST) rc = go_bwd_tiled<16, 8, 3, NCONV_LOAD_UPCAT_UP_FIRST>(d, a, part, nblk, tx, tc, st, why);
        else rc = go_bwd_tiled<8, 1, 1, NCONV_LOAD_PLAIN>(d, a, part, nblk, tx, tc, st, why);
    } else {
        if (a.gxa || a.gca || a.gxb || a.gcb) rc = launch_dgrad_generic(d, a, tx, tc, st, why);
        if (!rc && (a.gw || a.gb)) {
            const int fan = (L.Cin / L.groups) * L.KH * L.KW;
            rc = launch_wgrad_generic(d, a, part, nblk, st, why);
            if (!rc) rc = launch_wgrad_reduce(a, part, nblk, L.Cout * fan, L.Cout, fan, L.wsum, st, why);
        }
    }
    if (rc) return rc;
    // (dgrad_phase, the fused-tail layer's included, writes the upsampled half's gradient itself)
    if (is_upcat(L) && (a.gxb || a.gcb) && !(path == kTiled && dgrad_phase_ok(L)))
        launch_upsample_bwd_gather(d, a, tx, tc, st);
    return launch_status(why);
}

}  // namespace nconv
