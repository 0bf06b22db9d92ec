// nconv_dgrad.hip — exact-fp32 input-gradient ("dgrad") kernels of the NConv backward for gfx950
// and their launchers (the math: nconv_bwd.hip's header).
#include "nconv_internal.h"
#include "nconv_route.h"
#include "nconv_prologue.h"

namespace nconv {

constexpr int kT = 256;

// Staging of output-side planes {gN, gD} over an OHT x OWT halo tile (origin oh0, ow0) for the
// dgrad: the element map (LDS slot, byte offset in an output plane, or past-the-end for the zero
// padding) is computed once per workgroup; per output channel the four saved planes (gy, gcout,
// y, cout) are read with buffer loads and {gN, gD} are formed at store time. Elements are dealt
// to the 256 threads row-major; slots past the tile go to a dump slot after the plane.
// nconv7 (1x1, padding 2) consumer of this layer's outputs fused into its backward (T7): the
// layer's output gradient at (oh, ow) is nconv7's input gradient there, G_xc = w7[o] gN7, G_c =
// w7[o] gD7 with {gN7, gD7} from nconv7's (gy, y, cout) at (oh + 2, ow + 2); gy = G_xc * cout,
// gcout = G_c + G_xc * y (nconv7's dgrad_tiled<8,1,1> epilogue, same operations).
// (t7_off, t7_nd, t7_gy: nconv_internal.h)

// GC7 (with T7): nconv7's cout gradient is read too (BwdArgs t7gco), one more plane beside its gy.
template <int OHT, int OWT, int OWP, bool GP = false, bool T7 = false, bool GC7 = false>
struct GTileStager {
    static constexpr int N7 = GC7 ? 4 : 3;  // nconv7's gy, y, cout (+ gcout)
    static constexpr int NT = OHT * OWT;
    static constexpr int NE = (NT + 255) / 256;
    static constexpr int PLANE = OHT * OWP;
    static constexpr int PLANE_STRIDE = PLANE + 2;
    static constexpr int NV = GP ? 7 : 4;  // gy, gcout, y, cout (+ pooled gy, gcout, argmax code)
    static constexpr unsigned OOB = 0x80000000u;
    unsigned lofs[NE];
    unsigned go[NE];
    unsigned gpo[GP ? NE : 1];  // pooled element offsets, window slots (GP)
    unsigned gsub[GP ? NE : 1];
    float t7n[T7 ? NE : 1], t7d[T7 ? NE : 1];  // {gN7, gD7} per element (T7)

    __device__ __forceinline__ void init(const nconv_layer& L, int oh0, int ow0, int tid) {
#pragma unroll
        for (int k = 0; k < NE; ++k) {
            const int e = tid + 256 * k;
            const int r = e / OWT, col = e - r * OWT;
            const int oh = oh0 + r, ow = ow0 + col;
            const bool in = e < NT && (unsigned)oh < (unsigned)L.Ho && (unsigned)ow < (unsigned)L.Wo;
            lofs[k] = e < NT ? r * OWP + col : PLANE;
            go[k] = in ? (unsigned)(oh * L.Wo + ow) * 4u : OOB;
            if constexpr (GP) {
                gpo[k] = in ? pool_elem_off(oh, ow, L.Ho >> 1, L.Wo >> 1, OOB) : OOB;
                gsub[k] = (unsigned)(((oh & 1) << 1) | (ow & 1));
            }
        }
    }

    // T7: nconv7's (gy, y, cout [, gcout]) of the elements (loads issued here, {gN7, gD7} formed by t7_form)
    __device__ __forceinline__ void t7_load(const nconv_layer& L, const BwdArgs& a, int b, int oh0, int ow0, int tid,
                                            float (&v)[N7][NE]) const {
        const int pl7 = a.t7ph * a.t7pw;
        const size_t base = (size_t)b * pl7;
        const __amdgpu_buffer_rsrc_t rg = plane_rsrc(a.t7gy + base, pl7 * 4);
        const __amdgpu_buffer_rsrc_t ry = plane_rsrc(a.t7y + base, pl7 * 4);
        const __amdgpu_buffer_rsrc_t rc = plane_rsrc(a.t7co + base, pl7 * 4);
#pragma unroll
        for (int k = 0; k < NE; ++k) {
            const int e = tid + 256 * k;
            const int r = e / OWT, col = e - r * OWT;
            const unsigned off = e < NT ? t7_off(a, oh0 + r, ow0 + col, L.Ho, L.Wo, OOB) : OOB;
            v[0][k] = ld_f32(rg, off);
            v[1][k] = ld_f32(ry, off);
            v[2][k] = ld_f32(rc, off);
            if constexpr (GC7) v[N7 - 1][k] = ld_f32(plane_rsrc(a.t7gco + base, pl7 * 4), off);
        }
    }
    __device__ __forceinline__ void t7_form(const BwdArgs& a, const float (&v)[N7][NE]) {
#pragma unroll
        for (int k = 0; k < NE; ++k) {
            if constexpr (T7) t7_nd(a, v[0][k], GC7 ? v[N7 - 1][k] : 0.f, v[1][k], v[2][k], t7n[k], t7d[k]);
        }
    }

    // raw (gy, gcout, y, cout [, pooled gy, pooled gcout, code]) of output channel o of image b, no wait
    __device__ __forceinline__ void load(const nconv_layer& L, const BwdArgs& a, int b, int o,
                                         float (&v)[NV][NE]) const {
        const int plane = L.Ho * L.Wo;
        const size_t base = ((size_t)b * L.Cout + o) * plane;
        const __amdgpu_buffer_rsrc_t rgy = plane_rsrc(a.gy + base, plane * 4);
        const __amdgpu_buffer_rsrc_t ry = plane_rsrc(a.y + base, plane * 4);
        const __amdgpu_buffer_rsrc_t rco = plane_rsrc(a.co + base, plane * 4);
        if constexpr (T7) {  // gy / gcout are formed from nconv7's planes at store time
#pragma unroll
            for (int k = 0; k < NE; ++k) {
                v[2][k] = ld_f32(ry, go[k]);
                v[3][k] = ld_f32(rco, go[k]);
            }
            return;
        }
#pragma unroll
        for (int k = 0; k < NE; ++k) {
            v[0][k] = ld_f32(rgy, go[k]);
            v[2][k] = ld_f32(ry, go[k]);
            v[3][k] = ld_f32(rco, go[k]);
        }
        // gcout may be absent (= 0): a zero-sized resource then reads 0 -- no branch, since a branch
        // here makes the compiler wait for all of this stage's loads at the join, i.e. right after
        // issuing them instead of behind the next plane's FMAs
        const __amdgpu_buffer_rsrc_t rgc = plane_rsrc(a.gco ? a.gco + base : a.y, a.gco ? plane * 4 : 0);
#pragma unroll
        for (int k = 0; k < NE; ++k) v[1][k] = ld_f32(rgc, go[k]);
        if constexpr (GP) {
            const int pplane = (L.Ho >> 1) * (L.Wo >> 1);
            const size_t pbase = ((size_t)b * L.Cout + o) * pplane;
            const __amdgpu_buffer_rsrc_t rpy = plane_rsrc(a.gpy + pbase, pplane * 4);
            const __amdgpu_buffer_rsrc_t rpc = plane_rsrc(a.gpc + pbase, pplane * 4);
            const __amdgpu_buffer_rsrc_t rpa = plane_rsrc((const float*)(a.parg + pbase), pplane * 4);
#pragma unroll
            for (int k = 0; k < NE; ++k) {
                v[4][k] = ld_f32(rpy, gpo[k]);
                v[5][k] = ld_f32(rpc, gpo[k]);
                v[6][k] = ld_f32(rpa, gpo[k]);  // the code word, carried as raw bits until store
            }
        }
    }

    __device__ __forceinline__ void store(const nconv_layer& L, int o, const float (&v)[NV][NE], f2* t,
                                          float a_w7 = 0.f) const {
        const float bo = L.bias[o], so = L.wsum[o];
        const float w7 = T7 ? a_w7 : 0.f;
#pragma unroll
        for (int k = 0; k < NE; ++k) {
            float gy, gco;
            if constexpr (T7) {
                t7_gy(w7, t7n[k], t7d[k], v[2][k], v[3][k], gy, gco);
            } else {
                gy = v[0][k];
                gco = v[1][k];
            }
            if constexpr (GP) pool_route(gy, gco, v[4][k], v[5][k], __builtin_bit_cast(unsigned, v[6][k]), gsub[k]);
            float gN, gD;  // zero padding: gy = gcout = y = cout = 0 gives gN = gD = 0
            nconv_grad_nd(gy, gco, v[2][k], v[3][k], L.eps, bo, so, gN, gD);
            t[lofs[k]] = (f2){gN, gD};
        }
    }
};

// ---- dgrad: tiled, stride 1 ------------------------------------------------------------------------
template <int CIN, int K>
struct DgCfg {
    static constexpr int P = 2;  // input pixels per thread (f2 epilogue: any even width stays vectorized)
    static constexpr int TPR = 16, TW = TPR * P, TH = kT / TPR;
    static constexpr int OHT = TH + K - 1, OWT = TW + K - 1;
    static constexpr int OWP = (OWT + 1) & ~1;  // even pitch: 16-B aligned window reads
    static constexpr int NV = P + K - 1;
};

template <int P>
struct VecOf;
template <>
struct VecOf<4> { typedef f4 T; };
template <>
struct VecOf<2> { typedef f2 T; };

// ---- fused nconv1 weight gradient (training, exact fp32) ------------------------------------------
// nconv2's input gradient at a pixel p is nconv1's output gradient there (gy1 = G_xc*c1, gcout1 =
// G_c + G_xc*y1), and nconv1 (1 -> 8, 5x5, padding 2, on x0 = S, c0 = (S > 0.01)) has
//     gW1[o][kh][kw] = sum_p gN1[o](p) * S(p + (kh-2, kw-2)) * c0(...) + gD1[o](p) * c0(...)
// whose terms vanish unless c0 = 1 at the tap: a correlation over the ~5 % of pixels that hold a
// depth sample. Per tile: {gN1, gD1} of the 16 x 32 pixels (8 channels) into LDS, the samples of the
// tile's 20 x 36 window listed once (a deterministic block prefix sum), then thread (o, tap) sums
// over the list; plus the dense sums gb1 = sum gy1 and sum gcout1*cout1 (the normaliser's term).
// One partial row per workgroup (wgrad_reduce_sum / wgrad_finish reduce them, deferred or not):
// nconv1's input gradient G[1] is never written to HBM and nconv1 needs no backward kernel.
// (kHeadNw, kHeadStride: nconv_internal.h)

template <int CIN, int TH, int TW>
struct HeadLds {
    static constexpr int RH = TH + 4, RW = TW + 4, RN = RH * RW;  // the tile's 5x5-window region
    static constexpr int NPL = CIN / 2;  // {gN1, gD1} planes held at once (22 KB of LDS, not 38)
    static constexpr int F2 = NPL * TH * TW + RN;                 // {gN1, gD1} planes + sample list
};

template <int CIN, int TH, int TW>
__device__ void head_wgrad_epilogue(const LayerDev& d, const BwdArgs& a, int b, int ih0, int iw0, int ty, int tx,
                                    const f2 (&acc)[CIN][2], f2* smem) {
    static_assert(CIN == 8, "nconv1 has 8 output channels");
    using H = HeadLds<CIN, TH, TW>;
    constexpr int RW = H::RW, RN = H::RN;
    constexpr int NPL = H::NPL;
    f2* gn = smem;                                       // [NPL][TH][TW]
    f2* qlist = smem + NPL * TH * TW;                    // {row << 8 | col, S} of the samples
    f4 vh[CIN - NPL > 0 ? CIN - NPL : 1];                // the second half's {gN1, gD1} (NPL < CIN)
    __shared__ int wtot[4];
    __shared__ float red[4][2 * CIN];
    const nconv_layer& L = d.L;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int ih = ih0 + ty, iw = iw0 + tx;
    const bool pair = ih < L.H && iw + 1 < L.W && (L.W & 1) == 0;  // both pixels in range, 8-byte aligned
    float sgy[CIN], sgc[CIN];
#pragma unroll
    for (int i = 0; i < CIN; ++i) {
        sgy[i] = sgc[i] = 0.f;
        const size_t idx = plane_idx(b, i, L.a.C, L.a.H, L.a.W, ih < L.H ? ih : 0, iw < L.W ? iw : 0);
        float x[2] = {0.f, 0.f}, c[2] = {0.f, 0.f};
        if (pair) {
            const f2 xv = *reinterpret_cast<const f2*>(L.a.x + idx), cv = *reinterpret_cast<const f2*>(L.a.c + idx);
            x[0] = xv.x; x[1] = xv.y; c[0] = cv.x; c[1] = cv.y;
        } else {
#pragma unroll
            for (int j = 0; j < 2; ++j)
                if (ih < L.H && iw + j < L.W) {
                    x[j] = L.a.x[idx + j];
                    c[j] = L.a.c[idx + j];
                }
        }
        f2 v[2];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const bool ok = ih < L.H && iw + j < L.W;
            const float gy = acc[i][j].x * c[j], gco = acc[i][j].y + acc[i][j].x * x[j];
            float gN = 0.f, gD = 0.f;
            if (ok) {
                if (a.gxa) a.gxa[idx + j] = gy;  // G[1] only when asked for (the input gradient of S)
                if (a.gca) a.gca[idx + j] = gco;
                nconv_grad_nd(gy, gco, x[j], c[j], a.heps, a.hb[i], a.hs[i], gN, gD);
                sgy[i] += gy;
                sgc[i] = fmaf(gco, c[j], sgc[i]);
            }
            v[j] = (f2){gN, gD};
        }
        if (i < NPL) *reinterpret_cast<f4*>(gn + (i * TH + ty) * TW + tx) = (f4){v[0].x, v[0].y, v[1].x, v[1].y};
        else vh[i - NPL] = (f4){v[0].x, v[0].y, v[1].x, v[1].y};
    }
    // the depth samples (c0 = 1) of the window region, listed in (thread, element) order
    const float* Sp = a.hS + (size_t)b * L.H * L.W;
    constexpr int NE = (RN + kT - 1) / kT;
    float sv[NE];
    int cnt = 0;
#pragma unroll
    for (int k = 0; k < NE; ++k) {
        const int e = tid * NE + k;  // consecutive elements per thread: the list is row-major
        const int r = e / RW, cc = e - r * RW;
        const int qr = ih0 - 2 + r, qc = iw0 - 2 + cc;
        const bool in = e < RN && (unsigned)qr < (unsigned)L.H && (unsigned)qc < (unsigned)L.W;
        sv[k] = in ? Sp[(size_t)qr * L.W + qc] : 0.f;
        cnt += sv[k] > a.hthresh ? 1 : 0;
    }
    int total;
    int off = block_excl_scan<4>(cnt, wtot, total);
#pragma unroll
    for (int k = 0; k < NE; ++k) {
        if (sv[k] > a.hthresh) {
            const int e = tid * NE + k;
            qlist[off] = (f2){__builtin_bit_cast(float, ((e / RW) << 8) | (e % RW)), sv[k]};
            ++off;
        }
    }
    // dense sums: wave_ops.h's order
#pragma unroll
    for (int i = 0; i < CIN; ++i) sgy[i] = wave_sum(sgy[i]), sgc[i] = wave_sum(sgc[i]);
    if (lane == 0)
#pragma unroll
        for (int i = 0; i < CIN; ++i) {
            red[wv][i] = sgy[i];
            red[wv][CIN + i] = sgc[i];
        }
    __syncthreads();
    float* out = a.hpart + (size_t)blockIdx.x * kHeadStride;
    // thread (o, tap) sums its tap over the sample list; with NPL < CIN one half of the channels
    // at a time (the LDS of four planes instead of eight: more workgroups per CU)
    auto tap_sums = [&](int o0) __attribute__((always_inline)) {
        const int t = tid;
        if (t < NPL * 25) {
            const int ol = t / 25, tap = t - ol * 25, kh = tap / 5, kw = tap - kh * 5;
            const f2* g = gn + ol * TH * TW;
            float sn = 0.f, sd = 0.f;
            for (int n = 0; n < total; ++n) {
                const f2 q = qlist[n];
                const int qi = __builtin_bit_cast(int, q.x);
                const int pr = (qi >> 8) - kh, pc = (qi & 255) - kw;  // p = q - (tap - 2), region origin -2
                if ((unsigned)pr < (unsigned)TH && (unsigned)pc < (unsigned)TW) {
                    const f2 v = g[pr * TW + pc];
                    sn = fmaf(v.x, q.y, sn);
                    sd += v.y;
                }
            }
            out[o0 * 25 + t] = sn + sd;
        }
    };
    tap_sums(0);
    if (tid >= kHeadNw && tid < kHeadNw + 2 * CIN) {
        const int k = tid - kHeadNw;
        out[tid] = waves_in_order(&red[0][k], 2 * CIN);
    }
    if constexpr (NPL < CIN) {
        __syncthreads();  // every tap sum of the first half is done with its planes
#pragma unroll
        for (int i = NPL; i < CIN; ++i) *reinterpret_cast<f4*>(gn + ((i - NPL) * TH + ty) * TW + tx) = vh[i - NPL];
        __syncthreads();
        tap_sums(NPL);
    }
}

// One (output channel o, kernel row kh) step per iteration of the inner loop, not unrolled: its
// Cin*K weights ride SGPRs. The {gN, gD} planes of the output channels are staged one at a time
// into two LDS buffers, the loads two channels ahead (as the forward's input planes).
template <int CIN, int COUT, int K, int MODE, bool GP = false, bool HW = false>
__global__ __launch_bounds__(kT) void dgrad_tiled(LayerDev d, BwdArgs a, float* tmp_x, float* tmp_c) {
    using C = DgCfg<CIN, K>;
    using GS = GTileStager<C::OHT, C::OWT, C::OWP, GP>;
    constexpr int P = C::P;
    // with HW the staging planes' LDS is reused by the head epilogue ({gN1, gD1} planes + sample list)
    constexpr int TILE_F2 = HW && HeadLds<CIN, C::TH, C::TW>::F2 > 2 * GS::PLANE_STRIDE
                                ? HeadLds<CIN, C::TH, C::TW>::F2 : 2 * GS::PLANE_STRIDE;
    __shared__ __attribute__((aligned(16))) f2 tile[TILE_F2];
    const nconv_layer& L = d.L;
    const float* __restrict__ wgt = L.weight;
    const TileCoord tcd = xcd_tile((L.W + C::TW - 1) / C::TW, (L.H + C::TH - 1) / C::TH, L.B);
    const int tid = threadIdx.x, b = tcd.b;
    const int ih0 = tcd.ty * C::TH, iw0 = tcd.tx * C::TW;
    const int oh0 = ih0 + L.PH - (K - 1), ow0 = iw0 + L.PW - (K - 1);
    const int ty = tid / C::TPR, tx = (tid % C::TPR) * P;

    f2 acc[CIN][P];
#pragma unroll
    for (int i = 0; i < CIN; ++i)
#pragma unroll
        for (int j = 0; j < P; ++j) acc[i][j] = (f2){0.f, 0.f};

    auto fma_plane = [&](int o, int bufi) {
        const f2* row = &tile[bufi * GS::PLANE_STRIDE + (ty + K - 1) * C::OWP + tx];
        const float* wr = wgt + (size_t)o * CIN * K * K;
#pragma unroll 1
        for (int kh = 0; kh < K; ++kh, row -= C::OWP, wr += K) {
            f2 v[C::NV];
#pragma unroll
            for (int m = 0; m < C::NV / 2; ++m) {
                f4 qv = reinterpret_cast<const f4*>(row)[m];
                v[2 * m] = qv.xy;
                v[2 * m + 1] = qv.zw;
            }
            if constexpr (C::NV & 1) v[C::NV - 1] = row[C::NV - 1];
#pragma unroll
            for (int kw = 0; kw < K; ++kw)
#pragma unroll
                for (int i = 0; i < CIN; ++i) {
                    const float w = wr[i * K * K + kw];
                    const f2 w2 = (f2){w, w};
#pragma unroll
                    for (int j = 0; j < P; ++j)
                        acc[i][j] = __builtin_elementwise_fma(w2, v[j + K - 1 - kw], acc[i][j]);
                }
        }
    };

    GS gs;
    gs.init(L, oh0, ow0, tid);
    constexpr bool ONE = GP;
    float va[GS::NV][GS::NE], vb[ONE ? 1 : GS::NV][GS::NE];
    gs.load(L, a, b, 0, va);
    if constexpr (ONE) {
        // pooled stager (seven values per element): one plane ahead, one register set -- 85
        // instead of 105 VGPRs, five waves per SIMD instead of four (with the head epilogue's
        // 22 KB of LDS); nconv2's input gradient 353 -> 332 us alone, the graphed step within
        // noise (the weight gradients share the CUs), profiles/r5_ab_dgrad_occupancy.log
#pragma unroll 1
        for (int o = 0; o < COUT; ++o) {
            const int bufi = o & 1;
            gs.store(L, o, va, tile + bufi * GS::PLANE_STRIDE);
            __syncthreads();
            gs.load(L, a, b, o + 1 < COUT ? o + 1 : COUT - 1, va);
            fma_plane(o, bufi);
        }
    } else {
    if (COUT > 1) gs.load(L, a, b, 1, vb);
#pragma unroll 1
    for (int o = 0; o < COUT; o += 2) {
        gs.store(L, o, va, tile);
        __syncthreads();
        gs.load(L, a, b, o + 2 < COUT ? o + 2 : COUT - 1, va);  // unconditional (see fwd_tiled)
        fma_plane(o, 0);
        if (o + 1 < COUT) {
            gs.store(L, o + 1, vb, tile + GS::PLANE_STRIDE);
            __syncthreads();
            gs.load(L, a, b, o + 3 < COUT ? o + 3 : COUT - 1, vb);
            fma_plane(o + 1, 1);
        }
    }
    }

    // ---- epilogue: gx = G_xc*c, gc = G_c + G_xc*x, routed through the glue's backward ----
    if constexpr (HW) {  // nconv2's input gradient feeds nconv1's weight gradient in-tile
        static_assert(MODE == NCONV_LOAD_PLAIN && P == 2, "fused head weight gradient: plain 2-pixel tiles");
        __syncthreads();  // the staging tile is free
        if constexpr (HW) head_wgrad_epilogue<CIN, C::TH, C::TW>(d, a, b, ih0, iw0, ty, tx, acc, tile);
        return;
    }
    const int ih = ih0 + ty;
    if (ih >= L.H) return;
    const int iwb = iw0 + tx;
    const bool full = (L.W % P) == 0 && iwb + P <= L.W;  // P-aligned, fully in range
    const bool accm = a.accumulate != 0;
    typedef typename VecOf<P>::T V;
#pragma unroll
    for (int i = 0; i < CIN; ++i) {
        if constexpr (MODE == NCONV_LOAD_POOL2) {
            if (P == 2 && full && (L.a.W & 3) == 0) {
                // the two pooled pixels' 2x2 windows are 4 columns x 2 rows of the producer: 16-byte
                // loads of x / c for the argmax, 16-byte stores (or read-modify-writes) of gx / gc with
                // 0 at the other three slots (what the reference's max_pool2d backward adds there)
                const size_t W2 = (size_t)L.a.W;
                const size_t i0 = plane_idx(b, i, L.a.C, L.a.H, L.a.W, 2 * ih, 2 * iwb);
                const f4 x0 = *reinterpret_cast<const f4*>(L.a.x + i0);
                const f4 x1 = *reinterpret_cast<const f4*>(L.a.x + i0 + W2);
                const f4 c0 = *reinterpret_cast<const f4*>(L.a.c + i0);
                const f4 c1 = *reinterpret_cast<const f4*>(L.a.c + i0 + W2);
                f4 gx[2], gc[2];
#pragma unroll
                for (int j = 0; j < P; ++j) {
                    int ax, ac;
                    const float xm = pool4(x0[2 * j], x0[2 * j + 1], x1[2 * j], x1[2 * j + 1], ax);
                    const float cm = pool4(c0[2 * j], c0[2 * j + 1], c1[2 * j], c1[2 * j + 1], ac);
                    const float vx = acc[i][j].x * cm, vc = acc[i][j].y + acc[i][j].x * xm;
#pragma unroll
                    for (int s = 0; s < 4; ++s) {
                        gx[s >> 1][2 * j + (s & 1)] = (s == ax) ? vx : 0.f;
                        gc[s >> 1][2 * j + (s & 1)] = (s == ac) ? vc : 0.f;
                    }
                }
#pragma unroll
                for (int r = 0; r < 2; ++r) {
                    if (a.gxa) {
                        f4* p = reinterpret_cast<f4*>(a.gxa + i0 + r * W2);
                        *p = accm ? *p + gx[r] : gx[r];
                    }
                    if (a.gca) {
                        f4* p = reinterpret_cast<f4*>(a.gca + i0 + r * W2);
                        *p = accm ? *p + gc[r] : gc[r];
                    }
                }
                if (!accm)
#pragma unroll
                    for (int j = 0; j < P; ++j) pool_zero_leftovers(d, a, b, i, ih, iwb + j);
                continue;
            }
#pragma unroll
            for (int j = 0; j < P; ++j)
                if (iwb + j < L.W) {
                    route_grad<MODE>(d, a, b, i, ih, iwb + j, acc[i][j].x, acc[i][j].y, tmp_x, tmp_c);
                    if (!accm) pool_zero_leftovers(d, a, b, i, ih, iwb + j);
                }
        } else {
            const ChanSrc s = chan_src<MODE>(d, b, i);
            if (!full) {
#pragma unroll
                for (int j = 0; j < P; ++j)
                    if (iwb + j < L.W) route_grad<MODE>(d, a, b, i, ih, iwb + j, acc[i][j].x, acc[i][j].y, tmp_x, tmp_c);
                continue;
            }
            // vector path: P consecutive pixels of one row
            float x[P], c[P];
            if (s.kind == kUp) {
#pragma unroll
                for (int j = 0; j < P; ++j) load_chan(d, s, ih, iwb + j, x[j], c[j]);
            } else {
                const V xv = *reinterpret_cast<const V*>(s.x + ih * s.W + iwb);
#pragma unroll
                for (int j = 0; j < P; ++j) x[j] = xv[j];
                if (s.kind == kThresh) {
#pragma unroll
                    for (int j = 0; j < P; ++j) c[j] = (x[j] > L.thresh) ? 1.0f : 0.0f;
                } else {
                    const V cv = *reinterpret_cast<const V*>(s.c + ih * s.W + iwb);
#pragma unroll
                    for (int j = 0; j < P; ++j) c[j] = cv[j];
                }
            }
            V gxv, gcv;
#pragma unroll
            for (int j = 0; j < P; ++j) {
                gxv[j] = acc[i][j].x * c[j];
                gcv[j] = acc[i][j].y + acc[i][j].x * x[j];
            }
            float *gxp, *gcp;
            size_t off;
            bool acc_here = accm;
            if (s.kind == kUp) {  // upsampled channel: stage for upsample_bwd_gather
                const bool skip_first = (MODE == NCONV_LOAD_UPCAT_SKIP_FIRST);
                const int cb = skip_first ? i - L.a.C : i;
                off = plane_idx(b, cb, L.b.C, L.H, L.W, ih, iwb);
                gxp = tmp_x;
                gcp = tmp_c;
                acc_here = false;
            } else {
                const int ca = (MODE == NCONV_LOAD_UPCAT_UP_FIRST) ? i - L.b.C : i;
                off = plane_idx(b, ca, L.a.C, L.a.H, L.a.W, ih, iwb);
                gxp = a.gxa;
                gcp = (s.kind == kThresh) ? nullptr : a.gca;
            }
            if (gxp) {
                V* p = reinterpret_cast<V*>(gxp + off);
                *p = acc_here ? *p + gxv : gxv;
            }
            if (gcp) {
                V* p = reinterpret_cast<V*>(gcp + off);
                *p = acc_here ? *p + gcv : gcv;
            }
        }
    }
}

// ---- dgrad, phase form for an exactly 2x nearest-upsampled half (16 = 8 + 8 -> 8, 3x3, stride 1) ----
// The upsampled channels' input gradient is only needed summed over each 2x2 block (the
// nearest-upsample backward), and a block's sum is a 4x4 correlation of {gN, gD} with box-summed
// weights. Low pixel (lr, lc) of the tile covers full-resolution rows 2lr + e (e = 0, 1); staged
// output row 2lr + t receives input row 2lr + e through tap kh = e + 2 - t, so t = 0..3 collects the
// taps S(0) = {2}, S(1) = {1, 2}, S(2) = {0, 1}, S(3) = {0} (columns alike):
//     SG[i][lr][lc] = sum_o sum_{t,u} Wb[o][i][t][u] * g[o][2lr + t][2lc + u],  Wb = sum_{S(t) x S(u)} W
// 16 taps per low pixel instead of 4 x 9 per block, and the result goes straight to the producer's
// gradient (gx = SG_xc * c, gc = SG_c + SG_xc * x at the low pixel): no staged full-resolution plane,
// no gather kernel. The 8 skip channels run as in dgrad_tiled. Thread roles: 2 skip pixels x 8
// channels (dgrad_tiled's map) plus one low pixel x 4 upsampled channels, the channel half
// wave-uniform (waves 0-1 / 2-3) so the box weights stay scalar.
__global__ __launch_bounds__(kT) void box_weights(const float* __restrict__ w, int first_up, float* __restrict__ wb) {
    const int e = blockIdx.x * kT + threadIdx.x;  // [o][i][t][u], 8 x 8 x 4 x 4
    if (e < 1024) wb[e] = box_weight(w, first_up, e);
}

// The fused tail comes in two forms: T7 (nconv7's cout gradient is 0: nconv_bwd_ex) and T7C (it is
// read from BwdArgs t7gco: nconv_bwd_tail_conf), one or the other; TAIL below is either.
template <int MODE, bool T7 = false, bool T7C = false>
__global__ __launch_bounds__(kT) void dgrad_phase(LayerDev d, BwdArgs a, const float* __restrict__ wbox) {
    static_assert(!(T7 && T7C), "one form of the fused tail");
    constexpr bool TAIL = T7 || T7C;
    using C = DgCfg<16, 3>;
    using GS = GTileStager<C::OHT, C::OWT, C::OWP, false, TAIL, T7C>;
    constexpr int P = C::P, K = 3, CS = 8;
    constexpr int SK0 = (MODE == NCONV_LOAD_UPCAT_SKIP_FIRST) ? 0 : 8;  // first skip channel of W
    static_assert(C::TH % 2 == 0 && C::TW % 2 == 0 && C::OHT >= C::TH + 2 && C::OWT >= C::TW + 2, "low tile");
    __shared__ __attribute__((aligned(16))) f2 tile[2 * GS::PLANE_STRIDE];
    const nconv_layer& L = d.L;
    const float* __restrict__ wgt = L.weight;
    const TileCoord tcd = xcd_tile((L.W + C::TW - 1) / C::TW, (L.H + C::TH - 1) / C::TH, L.B);
    const int tid = threadIdx.x, b = tcd.b;
    const int ih0 = tcd.ty * C::TH, iw0 = tcd.tx * C::TW;
    const int oh0 = ih0 + L.PH - (K - 1), ow0 = iw0 + L.PW - (K - 1);
    const int ty = tid / C::TPR, tx = (tid % C::TPR) * P;
    const int half = __builtin_amdgcn_readfirstlane(tid >> 7);  // upsampled channels 4 half .. +3
    const int lq = tid & 127, lr = lq / (C::TW / 2), lc = lq % (C::TW / 2);
    static_assert((C::TH / 2) * (C::TW / 2) == 128, "one low pixel per thread and channel half");

    f2 acc[CS][P], au[4];
#pragma unroll
    for (int i = 0; i < CS; ++i)
#pragma unroll
        for (int j = 0; j < P; ++j) acc[i][j] = (f2){0.f, 0.f};
#pragma unroll
    for (int c = 0; c < 4; ++c) au[c] = (f2){0.f, 0.f};

    auto fma_plane = [&](int o, int bufi) {
        const f2* pl = &tile[bufi * GS::PLANE_STRIDE];
        const f2* row = pl + (ty + K - 1) * C::OWP + tx;
        const float* wr = wgt + ((size_t)o * 16 + SK0) * K * K;
#pragma unroll 1
        for (int kh = 0; kh < K; ++kh, row -= C::OWP, wr += K) {
            f2 v[C::NV];
#pragma unroll
            for (int m = 0; m < C::NV / 2; ++m) {
                const f4 qv = reinterpret_cast<const f4*>(row)[m];
                v[2 * m] = qv.xy;
                v[2 * m + 1] = qv.zw;
            }
#pragma unroll
            for (int kw = 0; kw < K; ++kw)
#pragma unroll
                for (int i = 0; i < CS; ++i) {
                    const float w = wr[i * K * K + kw];
                    const f2 w2 = (f2){w, w};
#pragma unroll
                    for (int j = 0; j < P; ++j)
                        acc[i][j] = __builtin_elementwise_fma(w2, v[j + K - 1 - kw], acc[i][j]);
                }
        }
        const f2* q = pl + (2 * lr) * C::OWP + 2 * lc;
        const float* wb = wbox + ((size_t)o * 8 + 4 * half) * 16;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const f4 q0 = reinterpret_cast<const f4*>(q + t * C::OWP)[0];
            const f4 q1 = reinterpret_cast<const f4*>(q + t * C::OWP)[1];
            const f2 g[4] = {q0.xy, q0.zw, q1.xy, q1.zw};
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const float w = wb[c * 16 + t * 4 + u];
                    au[c] = __builtin_elementwise_fma((f2){w, w}, g[u], au[c]);
                }
        }
    };

    GS gs;
    gs.init(L, oh0, ow0, tid);
    // one plane ahead with one register set (as dgrad_tiled's pooled stager): 79 instead of 109
    // VGPRs, six waves per SIMD instead of four; the tail's input gradient 235 -> 200 us alone
    // (profiles/r5_ab_dgrad_phase_one_ahead.log)
    float va[4][GS::NE];
    if constexpr (TAIL) {
        float v7[GS::N7][GS::NE];
        gs.t7_load(L, a, b, oh0, ow0, tid, v7);
        gs.load(L, a, b, 0, va);
        gs.t7_form(a, v7);
    } else {
        gs.load(L, a, b, 0, va);
    }
#pragma unroll 1
    for (int o = 0; o < 8; ++o) {
        const int bufi = o & 1;
        gs.store(L, o, va, tile + bufi * GS::PLANE_STRIDE, TAIL ? a.t7w[o] : 0.f);
        __syncthreads();
        gs.load(L, a, b, o + 1 < 8 ? o + 1 : 7, va);
        fma_plane(o, bufi);
    }

    const bool accm = a.accumulate != 0;
    // ---- upsampled half: the low pixel's gradient, straight into the producer's planes ----
    {
        const int lh = (ih0 >> 1) + lr, lw = (iw0 >> 1) + lc;
        if (lh < L.b.H && lw < L.b.W) {
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const size_t off = plane_idx(b, 4 * half + c, L.b.C, L.b.H, L.b.W, lh, lw);
                const float x = L.b.x[off], cf = L.b.c[off];
                if (a.gxb) put(a.gxb, off, au[c].x * cf, accm);
                if (a.gcb) put(a.gcb, off, au[c].y + au[c].x * x, accm);
            }
        }
    }
    // ---- skip half: gx = G_xc*c, gc = G_c + G_xc*x at full resolution ----
    const int ih = ih0 + ty, iwb = iw0 + tx;
    if (ih >= L.H) return;
    const bool full = (L.W % P) == 0 && iwb + P <= L.W;
#pragma unroll
    for (int i = 0; i < CS; ++i) {
        const size_t off = plane_idx(b, i, L.a.C, L.a.H, L.a.W, ih, iwb);
        if (full) {
            const f2 xv = *reinterpret_cast<const f2*>(L.a.x + off);
            const f2 cv = *reinterpret_cast<const f2*>(L.a.c + off);
            const f2 gxv = {acc[i][0].x * cv.x, acc[i][1].x * cv.y};
            const f2 gcv = {acc[i][0].y + acc[i][0].x * xv.x, acc[i][1].y + acc[i][1].x * xv.y};
            if (a.gxa) {
                f2* p = reinterpret_cast<f2*>(a.gxa + off);
                *p = accm ? *p + gxv : gxv;
            }
            if (a.gca) {
                f2* p = reinterpret_cast<f2*>(a.gca + off);
                *p = accm ? *p + gcv : gcv;
            }
        } else {
#pragma unroll
            for (int j = 0; j < P; ++j)
                if (iwb + j < L.W) {
                    const float x = L.a.x[off + j], cf = L.a.c[off + j];
                    if (a.gxa) put(a.gxa, off + j, acc[i][j].x * cf, accm);
                    if (a.gca) put(a.gca, off + j, acc[i][j].y + acc[i][j].x * x, accm);
                }
        }
    }
}

// the phase input gradient applies: exact fp32 backward of a DNET-shaped exactly-2x UpCat layer
bool dgrad_phase_ok(const nconv_layer& L) {
    if (!is_upcat(L) || L.bwd_math != NCONV_MATH_FP32) return false;
    if (L.Cin != 16 || L.Cout != 8 || L.a.C != 8 || L.b.C != 8 || L.KH != 3 || L.KW != 3) return false;
    if (L.SH != 1 || L.SW != 1 || L.DH != 1 || L.DW != 1 || L.groups != 1) return false;
    return L.a.H == L.H && L.a.W == L.W && L.H == 2 * L.b.H && L.W == 2 * L.b.W;
}

// ---- dgrad: generic (any stride / dilation / groups) ------------------------------------------------
template <int MODE>
__global__ __launch_bounds__(kT) void dgrad_generic(LayerDev d, BwdArgs a, float* tmp_x, float* tmp_c) {
    const nconv_layer& L = d.L;
    const size_t n = (size_t)L.B * L.Cin * L.H * L.W;
    const int cpg_in = L.Cin / L.groups, cpg_out = L.Cout / L.groups;
    for (size_t idx = (size_t)blockIdx.x * kT + threadIdx.x; idx < n; idx += (size_t)gridDim.x * kT) {
        const int iw = (int)(idx % L.W);
        const int ih = (int)((idx / L.W) % L.H);
        const int ci = (int)((idx / ((size_t)L.W * L.H)) % L.Cin);
        const int b = (int)(idx / ((size_t)L.W * L.H * L.Cin));
        const int g = ci / cpg_in, cl = ci - g * cpg_in;
        float Gxc = 0.f, Gc = 0.f;
        for (int ol = 0; ol < cpg_out; ++ol) {
            const int o = g * cpg_out + ol;
            const float bo = L.bias[o], so = L.wsum[o];
            for (int kh = 0; kh < L.KH; ++kh) {
                const int th = ih + L.PH - kh * L.DH;
                if (th < 0 || th % L.SH) continue;
                const int oh = th / L.SH;
                if (oh >= L.Ho) continue;
                for (int kw = 0; kw < L.KW; ++kw) {
                    const int tw = iw + L.PW - kw * L.DW;
                    if (tw < 0 || tw % L.SW) continue;
                    const int ow = tw / L.SW;
                    if (ow >= L.Wo) continue;
                    const size_t i = plane_idx(b, o, L.Cout, L.Ho, L.Wo, oh, ow);
                    float gN, gD;
                    nconv_grad_nd(a.gy[i], a.gco ? a.gco[i] : 0.f, a.y[i], a.co[i], L.eps, bo, so, gN, gD);
                    const float w = L.weight[(((size_t)o * cpg_in + cl) * L.KH + kh) * L.KW + kw];
                    Gxc = fmaf(w, gN, Gxc);
                    Gc = fmaf(w, gD, Gc);
                }
            }
        }
        route_grad<MODE>(d, a, b, ci, ih, iw, Gxc, Gc, tmp_x, tmp_c);
        if (MODE == NCONV_LOAD_POOL2 && !a.accumulate) pool_zero_leftovers(d, a, b, ci, ih, iw);
    }
}

// ---- nearest-upsample backward: low-res pixel gathers the high-res pixels that copied it -----------
__device__ __forceinline__ void up_range(int u, int in, int out, float scale, int& lo, int& hi) {
    if (out == in) { lo = u; hi = u + 1; return; }
    if (out == 2 * in) { lo = 2 * u; hi = 2 * u + 2; return; }
    int h = (int)floorf((float)u / scale) - 2;
    if (h < 0) h = 0;
    while (h < out && nearest_src(h, in, out, scale) < u) ++h;
    lo = h;
    while (h < out && nearest_src(h, in, out, scale) == u) ++h;
    hi = h;
}

__global__ __launch_bounds__(kT) void upsample_bwd_gather(LayerDev d, const float* tmp_x, const float* tmp_c,
                                                          float* gxb, float* gcb, int accumulate) {
    const nconv_layer& L = d.L;
    const int Cb = L.b.C, Hb = L.b.H, Wb = L.b.W;
    const size_t n = (size_t)L.B * Cb * Hb * Wb;
    for (size_t idx = (size_t)blockIdx.x * kT + threadIdx.x; idx < n; idx += (size_t)gridDim.x * kT) {
        const int v = (int)(idx % Wb);
        const int u = (int)((idx / Wb) % Hb);
        const size_t plane = idx / ((size_t)Wb * Hb);  // b*Cb + cb
        int h0, h1, w0, w1;
        up_range(u, Hb, L.H, d.up_scale_h, h0, h1);
        up_range(v, Wb, L.W, d.up_scale_w, w0, w1);
        float sx = 0.f, sc = 0.f;
        for (int h = h0; h < h1; ++h)
            for (int w = w0; w < w1; ++w) {
                const size_t i = (plane * L.H + h) * (size_t)L.W + w;
                sx += tmp_x[i];
                sc += tmp_c[i];
            }
        if (accumulate) {
            if (gxb) gxb[idx] += sx;
            if (gcb) gcb[idx] += sc;
        } else {
            if (gxb) gxb[idx] = sx;
            if (gcb) gcb[idx] = sc;
        }
    }
}

// ---- launchers --------------------------------------------------------------------------------------
size_t dgrad_blocks(const nconv_layer& L) {
    using D = DgCfg<8, 5>;  // the tile is the same for every layer shape
    return (size_t)((L.W + D::TW - 1) / D::TW) * ((L.H + D::TH - 1) / D::TH) * L.B;
}

template <int CIN, int COUT, int K, int MODE, bool GP, bool HW, bool T7>
int go_dgrad(const LayerDev& d, const BwdArgs& a, float* tx, float* tc, hipStream_t st, const char** why) {
    const nconv_layer& L = d.L;
    const dim3 g((unsigned)dgrad_blocks(L));  // see xcd_tile
    constexpr bool up = MODE == NCONV_LOAD_UPCAT_SKIP_FIRST || MODE == NCONV_LOAD_UPCAT_UP_FIRST;
    if constexpr (up && CIN == 16 && COUT == 8 && K == 3) {
        if (dgrad_phase_ok(L)) {  // box weights: the caller's, or into the (then unused) staging planes
            const float* wb = a.box;
            if (!wb) {
                hipLaunchKernelGGL(box_weights, dim3(1024 / kT), dim3(kT), 0, st, L.weight,
                                   MODE == NCONV_LOAD_UPCAT_SKIP_FIRST ? 8 : 0, tx);
                wb = tx;
            }
            if constexpr (T7)
                if (a.t7gco) {
                    hipLaunchKernelGGL((dgrad_phase<MODE, false, true>), g, dim3(kT), 0, st, d, a, wb);
                    return 0;
                }
            hipLaunchKernelGGL((dgrad_phase<MODE, T7>), g, dim3(kT), 0, st, d, a, wb);
        } else {
            hipLaunchKernelGGL((dgrad_tiled<CIN, COUT, K, MODE>), g, dim3(kT), 0, st, d, a, tx, tc);
        }
    } else {
        hipLaunchKernelGGL((dgrad_tiled<CIN, COUT, K, MODE, GP, HW>), g, dim3(kT), 0, st, d, a, tx, tc);
        if constexpr (HW) {  // nconv1's weight-gradient partial rows: one per dgrad workgroup
            if (a.defer) {
                *a.hnparts = (int)g.x;
            } else {
                const RedJob J{a.hpart, a.hs, a.hgw, a.hgb, (int)g.x, kHeadNw, 8, 25};
                return launch_wgrad_reduce_multi(1, &J, st, why);
            }
        }
    }
    return 0;
}

#define NCONV_GO_DGRAD(CIN, COUT, K, MODE, GP, HW, T7)                                                      \
    template int go_dgrad<CIN, COUT, K, MODE, GP, HW, T7>(const LayerDev&, const BwdArgs&, float*, float*, \
                                                          hipStream_t, const char**);
NCONV_GO_DGRAD(1, 8, 5, NCONV_LOAD_THRESH, false, false, false)
NCONV_GO_DGRAD(8, 8, 5, NCONV_LOAD_PLAIN, false, false, false)
NCONV_GO_DGRAD(8, 8, 5, NCONV_LOAD_PLAIN, true, false, false)
NCONV_GO_DGRAD(8, 8, 5, NCONV_LOAD_PLAIN, false, true, false)
NCONV_GO_DGRAD(8, 8, 5, NCONV_LOAD_PLAIN, true, true, false)
NCONV_GO_DGRAD(8, 8, 5, NCONV_LOAD_POOL2, false, false, false)
NCONV_GO_DGRAD(16, 8, 3, NCONV_LOAD_UPCAT_SKIP_FIRST, false, false, false)
NCONV_GO_DGRAD(16, 8, 3, NCONV_LOAD_UPCAT_UP_FIRST, false, false, false)
NCONV_GO_DGRAD(16, 8, 3, NCONV_LOAD_UPCAT_UP_FIRST, false, false, true)
NCONV_GO_DGRAD(8, 1, 1, NCONV_LOAD_PLAIN, false, false, false)
#undef NCONV_GO_DGRAD

static unsigned flat_blocks(size_t n) {
    const size_t blocks = (n + kT - 1) / kT;
    return (unsigned)(blocks > (1u << 20) ? 1u << 20 : blocks);
}

int launch_dgrad_generic(const LayerDev& d, const BwdArgs& a, float* tx, float* tc, hipStream_t st,
                         const char** why) {
    const nconv_layer& L = d.L;
    const unsigned blocks = flat_blocks((size_t)L.B * L.Cin * L.H * L.W);
    if (!blocks) return 0;
    switch (L.load_mode) {
#define NCONV_DG_GENERIC(M) \
    case M: hipLaunchKernelGGL(dgrad_generic<M>, dim3(blocks), dim3(kT), 0, st, d, a, tx, tc); return 0;
        NCONV_DG_GENERIC(NCONV_LOAD_PLAIN)
        NCONV_DG_GENERIC(NCONV_LOAD_THRESH)
        NCONV_DG_GENERIC(NCONV_LOAD_POOL2)
        NCONV_DG_GENERIC(NCONV_LOAD_UPCAT_SKIP_FIRST)
        NCONV_DG_GENERIC(NCONV_LOAD_UPCAT_UP_FIRST)
#undef NCONV_DG_GENERIC
    }
    *why = "unknown load mode";
    return -22;
}

void launch_upsample_bwd_gather(const LayerDev& d, const BwdArgs& a, const float* tx, const float* tc,
                                hipStream_t st) {
    const nconv_layer& L = d.L;
    const unsigned blocks = flat_blocks((size_t)L.B * L.b.C * L.b.H * L.b.W);
    if (blocks) hipLaunchKernelGGL(upsample_bwd_gather, dim3(blocks), dim3(kT), 0, st, d, tx, tc, a.gxb, a.gcb,
                                   a.accumulate);
}

}  // namespace nconv
