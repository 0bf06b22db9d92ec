// nconv_wgrad_mfma.hip — exact-fp32 weight gradient of the NConv backward on the gfx950 matrix
// cores: wgrad_mfma (one output row at a time), wgrad_mfma2 (output-row pairs), the g-row stager
// they share, and their launcher (the math: nconv_bwd.hip's header).
#include "nconv_internal.h"
#include "nconv_route.h"

namespace nconv {

constexpr int kT = 256;

// ---- wgrad on the matrix cores (fp32 MFMA 16x16x4, exact f32 products) -----------------------------
// For a 3x3 / 5x5 stride-1 layer the weight gradient is, per output row oh, a GEMM over the
// column index q = ow + kw:
//     gW[o][i][kh][kw] += sum_q  XC[i][oh+kh-PH][q-PW] * gN[o][oh][q-kw]
//                              +  C[i][oh+kh-PH][q-PW] * gD[o][oh][q-kw]
// with rows M = (kh, i) (i fastest) and columns N = (kw, o) (o fastest), K = q: the kernel-row
// shift lives in the A operand (which staged input row) and the kernel-column shift in the B
// operand (which g column), so neither operand is replicated per tap. A workgroup owns a 64-wide
// q strip of one image and walks a segment of output rows: a ring of K+1 staged input rows (one
// new row per output row, no halo re-staging) and a double-buffered {gN, gD} row with a K-1
// column left halo, one barrier per row, the next row's global loads issued before the current
// row's MFMAs. Each wave takes 16 of the 64 columns (4 MFMA k-steps per operand pair) and keeps the
// whole (M x N) tile in accumulators; the four waves' tiles are summed in a fixed order at the end
// into the block's partial row (then wgrad_reduce_sum / wgrad_finish, as for wgrad_tiled).
typedef float f4acc __attribute__((ext_vector_type(4)));

template <int CIN, int COUT, int K>
struct WmCfg {
    static constexpr int TW = 64;
    static constexpr int M = CIN * K, N = COUT * K;
    static constexpr int MT = (M + 15) / 16, NT = (N + 15) / 16;
    // LDS banks of the operand reads (ds_read_b32: bank = dword address mod 32, the two 32-lane
    // halves separate; a half holds k = lane >> 4 in {0, 1} (or {2, 3}) x 16 rows / columns):
    // A: row m = (kh, i) at slot(kh) * SLOT + i * XP + k. XP == 2 (mod 32) puts a kernel row's
    //    channels on 2i + k; for CIN = 8 a 16-row tile holds two kernel rows, in consecutive ring
    //    slots, and SLOT == 16 (mod 32) puts the second on the other 16 banks (the ring's wrap is an
    //    odd number of slots back, == 16 too), so every half reads 32 distinct banks.
    // B: column n = (kw, o) at o * GP + (K-1) - kw + k; lanes with equal o and k - kw read the same
    //    word (broadcast), so a half holds three words per channel, at 4o + {-1, 0, 1} + const with
    //    GP == 4 (mod 32): distinct. (Round 3 had pitches 68 / 72 laid out for 64 banks: 2-way on
    //    A, 4-way on B, ~4.5 K conflict cycles per wave in SQ_LDS_BANK_CONFLICT.)
    static constexpr int XP = TW + 2;
    static constexpr int SLOTS = K + 1;
    static constexpr int SKEW = (2 * CIN) % 32;
    static constexpr int SLOT = CIN * XP + (((SKEW - CIN * XP) % 32) + 32) % 32;
    static constexpr int GW = TW + K - 1;  // g row incl. the left halo
    static constexpr int GP = 68;          // == 4 (mod 32), see above
    static constexpr int ZB = 2;           // padded B columns read the zero row at banks 2, 3 (mod 4): free
    static_assert(GW <= GP, "g row pitch");
    static_assert(XP % 32 == 2 && GP % 32 == 4 && (CIN >= 16 || SLOT % 32 == 16), "bank layout");
    static_assert(COUT % 4 == 0, "g rows are staged four output channels per pass");
    // LDS (floats): xc ring + its zero row | c ring + its zero row | g [buf][part][COUT + 1 rows][GP]
    // (row COUT of each g part is zero). Padded M / N lanes read the zero rows, whose offsets from
    // the xc / gN data equal the c / gD part offsets, so one address per operand serves both parts.
    static constexpr int XR = SLOTS * SLOT;             // the zero row of the xc ring
    static constexpr int C_OFF = XR + GP;               // c ring (its zero row at C_OFF + XR)
    static constexpr int G_OFF = 2 * C_OFF;
    static constexpr int GPART = (COUT + 1) * GP;       // one part of one g buffer
    static constexpr int GBUF = 2 * GPART;
    static constexpr int STAGE = G_OFF + 2 * GBUF;
    static constexpr int RED = 4 * MT * NT * 256;
    static constexpr int LDS = STAGE > RED ? STAGE : RED;
    static constexpr int CPW = (CIN + 3) / 4, OPW = COUT / 4;  // channels staged per wave
};

constexpr int kWmWaves = 3;      // waves per SIMD asked of the compiler (wgrad_mfma)
constexpr int kWmStoreStep = 1;  // after which k-step the next row's staging is stored (its loads' latency budget)

// Staging of one {gN, gD} row of a strip for wgrad_mfma / wgrad_mfma2: COUT channels x 64 + K-1
// columns from column ow0 - (K-1), wave w taking channels w + 4 kk. A main pass (column = lane) per
// channel and one halo pass over all of them -- lane l < OPW (K-1) takes channel w + 4 (l / (K-1))
// at column 64 + l % (K-1) -- instead of a second pass per channel with K-1 of 64 lanes active;
// one buffer resource per image (the channel's plane offset in soffset for the main pass, in the
// lane's offset for the halo). load() issues a row's global loads without waiting; store() forms
// {gN, gD} (GP: pooled gradients routed in; T7: gy / gcout from nconv7's planes), writes channel o
// to row + o * PITCH (gD gpart floats on) and adds the strip's own columns (lanes >= K-1 and the
// halo) to the bias / normaliser sums that finish() reduces. A row that is not valid
// (wgrad_mfma2's padding of an odd last row) loads and stores zeros. GC7 (with T7): nconv7's cout
// gradient (BwdArgs t7gco) is read beside its gy, and the strip's sum of gcout * cout over its own
// pixels goes to nconv7's partial row (its normaliser term, applied by wgrad_finish).
template <int COUT, int K, int PITCH, bool GP, bool T7, bool GC7 = false>
struct GRowStager {
    static constexpr int N7 = GC7 ? 4 : 3;
    static constexpr int OPW = COUT / 4;
    static constexpr int NG = GP ? 7 : 4;  // gy, gco, y, cout (+ pooled gy, gcout, argmax code)
    static constexpr int NH = OPW * (K - 1);
    static_assert(COUT % 4 == 0 && NH <= 64, "four channels per pass, halo lanes");
    static constexpr unsigned OOB = 0x80000000u;
    int b, w, lane, ow0, plane, pplane;  // (pplane: the 2x2-pooled plane, GP)
    bool hl;
    int hkk, hcol, ho;
    float gq[OPW][NG], gh[NG];
    float g7[T7 ? 2 : 1][N7];                          // nconv7's gy, y, cout [, gcout] (T7): main, halo
    float gs7[1];                                      // nconv7's sum gcout * cout (GC7)
    float w7n[T7 ? OPW : 1], w7d[T7 ? OPW : 1];        // nconv7's weight-gradient sums
    float w7nh, w7dh;
    float gb_acc[OPW], gs_acc[OPW], gb_h, gs_h;
    // the wave's output channels' bias and normaliser, read once (not per row: a load right before
    // its use would put a global-memory round trip into every row)
    float bias_o[OPW], wsum_o[OPW], w7_o[T7 ? OPW : 1];

    __device__ __forceinline__ void init(const nconv_layer& L, const BwdArgs& a, int b_, int w_, int lane_, int ow0_) {
        b = b_, w = w_, lane = lane_, ow0 = ow0_;
        plane = L.Ho * L.Wo, pplane = (L.Ho >> 1) * (L.Wo >> 1);
        hl = lane < NH;
        hkk = hl ? lane / (K - 1) : 0, hcol = 64 + lane % (K - 1), ho = w + 4 * hkk;
        w7nh = w7dh = gb_h = gs_h = gs7[0] = 0.f;
#pragma unroll
        for (int kk = 0; kk < OPW; ++kk) {
            gb_acc[kk] = gs_acc[kk] = 0.f;
            bias_o[kk] = L.bias[w + 4 * kk];
            wsum_o[kk] = L.wsum[w + 4 * kk];
            if constexpr (T7) {
                w7n[kk] = w7d[kk] = 0.f;
                w7_o[kk] = a.t7w[w + 4 * kk];
            }
        }
    }

    __device__ __forceinline__ void load(const nconv_layer& L, const BwdArgs& a, int oh, bool valid) {
        const int ow = ow0 - (K - 1) + lane, owh = ow0 - (K - 1) + hcol;
        const bool row_in = valid && (unsigned)oh < (unsigned)L.Ho;
        const bool in = row_in && (unsigned)ow < (unsigned)L.Wo;
        const bool inh = hl && row_in && (unsigned)owh < (unsigned)L.Wo;
        if constexpr (T7) {
            const int pl7 = a.t7ph * a.t7pw;
            const size_t base7 = (size_t)b * pl7;
            const __amdgpu_buffer_rsrc_t r7g = plane_rsrc(a.t7gy + base7, pl7 * 4);
            const __amdgpu_buffer_rsrc_t r7y = plane_rsrc(a.t7y + base7, pl7 * 4);
            const __amdgpu_buffer_rsrc_t r7c = plane_rsrc(a.t7co + base7, pl7 * 4);
            const unsigned o0 = valid ? t7_off(a, oh, ow, L.Ho, L.Wo, OOB) : OOB;
            const unsigned o1 = valid && hl ? t7_off(a, oh, owh, L.Ho, L.Wo, OOB) : OOB;
            g7[0][0] = ld_f32(r7g, o0);
            g7[0][1] = ld_f32(r7y, o0);
            g7[0][2] = ld_f32(r7c, o0);
            g7[1][0] = ld_f32(r7g, o1);
            g7[1][1] = ld_f32(r7y, o1);
            g7[1][2] = ld_f32(r7c, o1);
            if constexpr (GC7) {
                const __amdgpu_buffer_rsrc_t r7q = plane_rsrc(a.t7gco + base7, pl7 * 4);
                g7[0][N7 - 1] = ld_f32(r7q, o0);
                g7[1][N7 - 1] = ld_f32(r7q, o1);
            }
        }
        const size_t base = (size_t)b * COUT * plane;
        const int bytes = COUT * plane * 4;
        const __amdgpu_buffer_rsrc_t rgy = plane_rsrc(a.gy + base, bytes);
        const __amdgpu_buffer_rsrc_t rco = plane_rsrc(a.co + base, bytes);
        const __amdgpu_buffer_rsrc_t ry = plane_rsrc(a.y + base, bytes);
        const __amdgpu_buffer_rsrc_t rgc = plane_rsrc(a.gco ? a.gco + base : a.y, a.gco ? bytes : 0);
        const unsigned off = in ? (unsigned)(oh * L.Wo + ow) * 4u : OOB;
        const unsigned offh = inh ? (unsigned)((ho * L.Ho + oh) * L.Wo + owh) * 4u : OOB;
#pragma unroll
        for (int kk = 0; kk < OPW; ++kk) {
            const int so = (w + 4 * kk) * plane * 4;
            if constexpr (!T7) gq[kk][0] = ld_f32s(rgy, off, so);  // (T7: gy, gcout formed at store time)
            gq[kk][1] = ld_f32s(rco, off, so);
            gq[kk][2] = ld_f32s(ry, off, so);
            if constexpr (!T7) gq[kk][3] = ld_f32s(rgc, off, so);
        }
        if constexpr (!T7) gh[0] = ld_f32(rgy, offh);
        gh[1] = ld_f32(rco, offh);
        gh[2] = ld_f32(ry, offh);
        if constexpr (!T7) gh[3] = ld_f32(rgc, offh);
        if constexpr (GP) {
            const int Hp = L.Ho >> 1, Wp = L.Wo >> 1;
            const size_t pbase = (size_t)b * COUT * pplane;
            const int pbytes = COUT * pplane * 4;
            const __amdgpu_buffer_rsrc_t rpy = plane_rsrc(a.gpy + pbase, pbytes);
            const __amdgpu_buffer_rsrc_t rpc = plane_rsrc(a.gpc + pbase, pbytes);
            const __amdgpu_buffer_rsrc_t rpa = plane_rsrc((const float*)(a.parg + pbase), pbytes);
            const unsigned po = in ? pool_elem_off(oh, ow, Hp, Wp, OOB) : OOB;
            const unsigned pe = inh ? pool_elem_off(oh, owh, Hp, Wp, OOB) : OOB;
            const unsigned poh = pe != OOB ? pe + (unsigned)(ho * pplane) * 4u : OOB;
#pragma unroll
            for (int kk = 0; kk < OPW; ++kk) {
                const int so = (w + 4 * kk) * pplane * 4;
                gq[kk][4] = ld_f32s(rpy, po, so);
                gq[kk][5] = ld_f32s(rpc, po, so);
                gq[kk][6] = ld_f32s(rpa, po, so);
            }
            gh[4] = ld_f32(rpy, poh);
            gh[5] = ld_f32(rpc, poh);
            gh[6] = ld_f32(rpa, poh);
        }
    }

    // one element: its loaded values v -> (gy, gco) and {gN, gD}; n7, d7: nconv7's {gN7, gD7} there
    // (T7), sub: its slot in the 2x2 pooling window (GP)
    __device__ __forceinline__ void form(const nconv_layer& L, const float (&v)[NG], float w7, float n7, float d7,
                                         unsigned sub, float bo, float so, float& gy, float& gco, float& gN,
                                         float& gD) const {
        if constexpr (T7) {
            t7_gy(w7, n7, d7, v[2], v[1], gy, gco);
        } else {
            gy = v[0];
            gco = v[3];
        }
        if constexpr (GP) pool_route(gy, gco, v[4], v[5], __builtin_bit_cast(unsigned, v[6]), sub);
        nconv_grad_nd(gy, gco, v[2], v[1], L.eps, bo, so, gN, gD);
    }

    __device__ __forceinline__ void store(const nconv_layer& L, const BwdArgs& a, float* row, int gpart, int oh_cur,
                                          bool valid) {
        float n7[2] = {0.f, 0.f}, d7[2] = {0.f, 0.f};
        if constexpr (T7)
#pragma unroll
            for (int p = 0; p < 2; ++p)
                t7_nd(a, g7[p][0], GC7 ? g7[p][N7 - 1] : 0.f, g7[p][1], g7[p][2], n7[p], d7[p]);
        // GC7: each of the strip's own pixels once -- the main columns, the halo lanes of channel slot 0.
        // INVARIANT: nconv7's planes have one channel, so every wave's g7 holds the same pixels of this row
        // (load() indexes them by lane alone, not by the wave's channels); each wave therefore carries the
        // same sum and finish() writes wave 0's. Staging g7 per wave would need a sum over the waves there.
        // (Guarding this with the wave index instead costs a live SGPR across the row loop: see finish().)
        if constexpr (GC7) {
            if (lane >= K - 1) gs7[0] = fmaf(g7[0][N7 - 1], g7[0][2], gs7[0]);
            if (hl && hkk == 0) gs7[0] = fmaf(g7[1][N7 - 1], g7[1][2], gs7[0]);
        }
        // the 2x2 window slot of the main / halo column (pooled-gradient routing)
        const unsigned sub = (unsigned)((oh_cur & 1) << 1), ow_m = (unsigned)(ow0 - (K - 1) + lane);
        const unsigned ow_h = (unsigned)(ow0 - (K - 1) + hcol);
#pragma unroll
        for (int kk = 0; kk < OPW; ++kk) {
            if constexpr (T7)
                if (lane >= K - 1) {  // nconv7's weight gradient: corr(x*c, gN7) + corr(c, gD7)
                    w7n[kk] = fmaf(gq[kk][2] * gq[kk][1], n7[0], w7n[kk]);
                    w7d[kk] = fmaf(gq[kk][1], d7[0], w7d[kk]);
                }
            float gy, gco, gN, gD;
            form(L, gq[kk], T7 ? w7_o[kk] : 0.f, n7[0], d7[0], sub | (ow_m & 1u), bias_o[kk], wsum_o[kk], gy, gco, gN,
                 gD);
            float* g = row + (w + 4 * kk) * PITCH + lane;
            g[0] = valid ? gN : 0.f;
            g[gpart] = valid ? gD : 0.f;
            if (lane >= K - 1) {  // this strip's own columns (an invalid row loaded zeros: gy = gco = 0)
                gb_acc[kk] += gy;
                gs_acc[kk] = fmaf(gco, gq[kk][1], gs_acc[kk]);
            }
        }
        {   // halo pass (columns 64 .. 64+K-2, all the strip's own)
            float bo = bias_o[0], so = wsum_o[0], w7 = T7 ? w7_o[0] : 0.f;
#pragma unroll
            for (int kk = 1; kk < OPW; ++kk) {
                bo = hkk == kk ? bias_o[kk] : bo;
                so = hkk == kk ? wsum_o[kk] : so;
                if constexpr (T7) w7 = hkk == kk ? w7_o[kk] : w7;
            }
            float gy, gco, gN, gD;
            form(L, gh, w7, n7[1], d7[1], sub | (ow_h & 1u), bo, so, gy, gco, gN, gD);
            if (hl) {
                float* g = row + ho * PITCH + hcol;
                g[0] = valid ? gN : 0.f;
                g[gpart] = valid ? gD : 0.f;
            }
            gb_h += gy;
            gs_h = fmaf(gco, gh[1], gs_h);
            if constexpr (T7) {
                w7nh = fmaf(gh[2] * gh[1], n7[1], w7nh);
                w7dh = fmaf(gh[1], d7[1], w7dh);
            }
        }
    }

    // the wave's channels' sums (the halo lanes' added before the butterfly) -> sums[o] = sum gy,
    // sums[COUT + o] = sum gcout*cout; T7: nconv7's partial row -- 8 weights, then its (unused) sum
    // gy slot and its sum gcout*cout (0 without GC7)
    __device__ __forceinline__ void finish(const BwdArgs& a, float* sums) const {
        // (the wave index read afresh: held from init() it is spilled across the row loop)
        const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
#pragma unroll
        for (int kk = 0; kk < OPW; ++kk) {
            const bool mine = hl && hkk == kk;  // the halo lanes' sums of this channel
            const float sb = wave_sum(gb_acc[kk] + (mine ? gb_h : 0.f));
            const float ss = wave_sum(gs_acc[kk] + (mine ? gs_h : 0.f));
            if (lane == 0) {
                sums[w + 4 * kk] = sb;
                sums[COUT + w + 4 * kk] = ss;
            }
        }
        if constexpr (T7) {
            float* o7 = a.t7part + (size_t)blockIdx.x * 10;
#pragma unroll
            for (int kk = 0; kk < OPW; ++kk) {
                const bool mine = hl && hkk == kk;
                const float sn = wave_sum(w7n[kk] + (mine ? w7nh : 0.f));
                const float sd = wave_sum(w7d[kk] + (mine ? w7dh : 0.f));
                if (lane == 0) o7[w + 4 * kk] = sn + sd;
            }
            if constexpr (GC7) {  // wave 0's sum: all four waves hold the same one (store()'s invariant)
                const float sg = wave_sum(gs7[0]);
                if (threadIdx.x == 0) o7[8] = 0.f, o7[9] = sg;
            } else {
                if (threadIdx.x < 2) o7[8 + threadIdx.x] = 0.f;
            }
        }
    }
};

// wgrad_mfma: the 16 -> 8 3x3 UpCat layers, with and without the fused nconv7 backward (T7); the
// 8 -> 8 5x5 layers take wgrad_mfma2 below.
// The fused tail comes in two forms, as in dgrad_phase: T7 (nconv7's cout gradient is 0) and T7C (it
// is read from BwdArgs t7gco), one or the other.
template <int CIN, int COUT, int K, int MODE, bool T7 = false, bool T7C = false>
__global__ __launch_bounds__(kT) __attribute__((amdgpu_waves_per_eu(kWmWaves, 8))) void wgrad_mfma(
    LayerDev d, BwdArgs a, float* part, int nstrip, int nseg, int seg_rows) {
    static_assert(!(T7 && T7C), "one form of the fused tail");
    static_assert(CIN == 16 && COUT == 8 && K == 3 &&
                      (MODE == NCONV_LOAD_UPCAT_SKIP_FIRST || MODE == NCONV_LOAD_UPCAT_UP_FIRST),
                  "wgrad_mfma: the 16 -> 8 3x3 upsample-concat layers");
    using C = WmCfg<CIN, COUT, K>;
    using GS = GRowStager<COUT, K, C::GP, false, T7 || T7C, T7C>;
    __shared__ __attribute__((aligned(16))) float lds[C::LDS];
    const nconv_layer& L = d.L;
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);  // wave-uniform: channel sources stay in SGPRs
    int blk = blockIdx.x;
    const int strip = blk % nstrip;
    blk /= nstrip;
    const int seg = blk % nseg, b = blk / nseg;
    const int ow0 = strip * C::TW;
    const int r0 = seg * seg_rows, r1 = min(L.Ho, r0 + seg_rows);
    constexpr unsigned OOB = 0x80000000u;

    for (int e = tid; e < C::GP; e += kT) {
        lds[C::XR + e] = 0.f;
        lds[C::C_OFF + C::XR + e] = 0.f;
#pragma unroll
        for (int z = 0; z < 4; ++z) lds[C::G_OFF + z * C::GPART + COUT * C::GP + e] = 0.f;
    }

    // per-lane MFMA operand coordinates (A[m = lane&15][k = lane>>4], B[k = lane>>4][n = lane&15])
    const int kq = lane >> 4, ml = lane & 15;
    int a_kh[C::MT], a_ik[C::MT], b_off[C::NT];
#pragma unroll
    for (int t = 0; t < C::MT; ++t) {
        const int m = 16 * t + ml;
        a_kh[t] = m < C::M ? m / CIN : -1;
        a_ik[t] = (m % CIN) * C::XP + kq;
    }
#pragma unroll
    for (int u = 0; u < C::NT; ++u) {
        const int n = 16 * u + ml;
        b_off[u] = n < C::N ? (n % COUT) * C::GP + (K - 1) - n / COUT + kq : COUT * C::GP + C::ZB + kq;
    }

    // ---- staging: one input row (CIN x 64 columns) and one g row (COUT x (64+K-1) columns) ----
    float px[C::CPW], pc[C::CPW];

    // UpCat inputs: the wave's channel sources, the up plane's column map and one resource per
    // source image resolved once, not per row (per-row channel resolution cost ~100 SGPR-spill
    // reloads and a general nearest-index path per row); per row only the row map and two offsets.
    const int iw_in = ow0 - L.PW + lane;
    const bool col_in = (unsigned)iw_in < (unsigned)L.W;
    const int sw_up = nearest_src(col_in ? iw_in : 0, L.b.W, L.W, d.up_scale_w);
    bool up_k[C::CPW];
    int so_k[C::CPW];
#pragma unroll
    for (int kk = 0; kk < C::CPW; ++kk) {
        const int i = w + 4 * kk;
        const bool skip_first = MODE == NCONV_LOAD_UPCAT_SKIP_FIRST;
        const int first_c = skip_first ? L.a.C : L.b.C;
        const bool from_a = skip_first ? (i < first_c) : (i >= first_c);
        up_k[kk] = !from_a;
        so_k[kk] = (from_a ? (skip_first ? i : i - first_c) * L.a.H * L.a.W
                           : (skip_first ? i - first_c : i) * L.b.H * L.b.W) * 4;
    }
    const int abytes = L.a.C * L.a.H * L.a.W * 4, bbytes = L.b.C * L.b.H * L.b.W * 4;
    const float* ax_img = L.a.x + (size_t)b * L.a.C * L.a.H * L.a.W;
    const float* ac_img = L.a.c + (size_t)b * L.a.C * L.a.H * L.a.W;
    const float* bx_img = L.b.x + (size_t)b * L.b.C * L.b.H * L.b.W;
    const float* bc_img = L.b.c + (size_t)b * L.b.C * L.b.H * L.b.W;
    auto load_in = [&](int ih) {
        const bool in = (unsigned)ih < (unsigned)L.H && col_in;
        const int sh = nearest_src(in ? ih : 0, L.b.H, L.H, d.up_scale_h);
        const unsigned od = in ? (unsigned)(ih * L.a.W + iw_in) * 4u : OOB;
        const unsigned ou = in ? (unsigned)(sh * L.b.W + sw_up) * 4u : OOB;
#pragma unroll
        for (int kk = 0; kk < C::CPW; ++kk) {
            const int i = w + 4 * kk;
            px[kk] = pc[kk] = 0.f;
            if (i < CIN) {
                const bool up = up_k[kk];
                const __amdgpu_buffer_rsrc_t rx = plane_rsrc(up ? bx_img : ax_img, up ? bbytes : abytes);
                const __amdgpu_buffer_rsrc_t rc = plane_rsrc(up ? bc_img : ac_img, up ? bbytes : abytes);
                px[kk] = ld_f32s(rx, up ? ou : od, so_k[kk]);
                pc[kk] = ld_f32s(rc, up ? ou : od, so_k[kk]);
            }
        }
    };
    auto store_in = [&](int ih) {
        const int slot = ((ih % C::SLOTS) + C::SLOTS) % C::SLOTS;
#pragma unroll
        for (int kk = 0; kk < C::CPW; ++kk) {
            const int i = w + 4 * kk;
            if (i < CIN) {
                lds[slot * C::SLOT + i * C::XP + lane] = px[kk] * pc[kk];
                lds[C::C_OFF + slot * C::SLOT + i * C::XP + lane] = pc[kk];
            }
        }
    };
    GS gs;
    gs.init(L, a, b, w, lane, ow0);
    float* const grow = lds + C::G_OFF;  // {gN, gD} rows [buf][part][COUT + 1][GP]

    f4acc acc[C::MT][C::NT];
#pragma unroll
    for (int t = 0; t < C::MT; ++t)
#pragma unroll
        for (int u = 0; u < C::NT; ++u) acc[t][u] = (f4acc){0.f, 0.f, 0.f, 0.f};

    // The next row is staged DURING this row's MFMAs (its loads before the first half of the k-steps,
    // its stores after it): its input row goes to the ring slot this row does not read (K + 1 slots,
    // K in use), its g row to the other buffer (whose last reader, the previous row, is behind the
    // barrier) -- one barrier per row, and the staging's VALU work interleaved with the MFMAs
    // instead of between barriers.
    if (r0 < r1) {
        for (int kh = 0; kh < K; ++kh) {  // prologue: the segment's first K input rows and g row
            load_in(r0 - L.PH + kh);
            store_in(r0 - L.PH + kh);
        }
        gs.load(L, a, r0, true);
        gs.store(L, a, grow, C::GPART, r0, true);
    }
    __syncthreads();
#pragma unroll 1
    for (int oh = r0; oh < r1; ++oh) {
        const int buf = (oh - r0) & 1;
        const bool more = oh + 1 < r1;
        int ax[C::MT], bn[C::NT];
#pragma unroll
        for (int t = 0; t < C::MT; ++t) {
            const int ih = oh - L.PH + a_kh[t];
            const int slot = ((ih % C::SLOTS) + C::SLOTS) % C::SLOTS;
            ax[t] = a_kh[t] < 0 ? C::XR + kq : slot * C::SLOT + a_ik[t];
        }
#pragma unroll
        for (int u = 0; u < C::NT; ++u) bn[u] = C::G_OFF + buf * C::GBUF + b_off[u];
        if (more) {
            load_in(oh + 1 - L.PH + K - 1);
            gs.load(L, a, oh + 1, true);
        }
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int q0 = 16 * w + 4 * s;
#pragma unroll
            for (int part = 0; part < 2; ++part) {  // {x*c, gN} then {c, gD}
                float va[C::MT], vb[C::NT];
#pragma unroll
                for (int t = 0; t < C::MT; ++t) va[t] = lds[ax[t] + part * C::C_OFF + q0];
#pragma unroll
                for (int u = 0; u < C::NT; ++u) vb[u] = lds[bn[u] + part * C::GPART + q0];
#pragma unroll
                for (int t = 0; t < C::MT; ++t)
#pragma unroll
                    for (int u = 0; u < C::NT; ++u)
                        acc[t][u] = __builtin_amdgcn_mfma_f32_16x16x4f32(va[t], vb[u], acc[t][u], 0, 0, 0);
            }
            if (s == kWmStoreStep && more) {
                store_in(oh + 1 - L.PH + K - 1);
                gs.store(L, a, grow + (buf ^ 1) * C::GBUF, C::GPART, oh + 1, true);
            }
        }
        __syncthreads();
    }

    // ---- the four waves' tiles summed in a fixed order -> this block's partial row ----
    constexpr int NW = COUT * CIN * K * K;
    constexpr int NE = C::MT * C::NT * 256;
    float* out = part + (size_t)blockIdx.x * (NW + 2 * COUT);
    __syncthreads();
#pragma unroll
    for (int t = 0; t < C::MT; ++t)
#pragma unroll
        for (int u = 0; u < C::NT; ++u)
#pragma unroll
            for (int r = 0; r < 4; ++r) lds[w * NE + (t * C::NT + u) * 256 + r * 64 + lane] = acc[t][u][r];
    __syncthreads();
    for (int e = tid; e < NE; e += kT) {
        const float v = ((lds[e] + lds[NE + e]) + lds[2 * NE + e]) + lds[3 * NE + e];
        const int l = e & 63, r = (e >> 6) & 3, tu = e >> 8;
        const int u = tu % C::NT, t = tu / C::NT;
        const int m = 16 * t + (l >> 4) * 4 + r, n = 16 * u + (l & 15);
        if (m < C::M && n < C::N) {
            const int kh = m / CIN, i = m % CIN, kw = n / COUT, o = n % COUT;
            out[((o * CIN + i) * K + kh) * K + kw] = v;
        }
    }
    gs.finish(a, out + NW);
}

// ---- wgrad_mfma over output-row pairs (8 -> 8, 5x5: nconv2 and the down layers) ------------------
// wgrad_mfma's (kh, i) x (kw, o) tile is 40 x 40 for these layers and pads to 48 x 48 (3 x 3 MFMA
// tiles, 69 % of the products useful). Two output rows oh, oh + 1 at once fill the tiles exactly:
// rows M = (r, i), r = 0..K over the K + 1 staged input rows oh - PH + r (48 = 3 tiles), columns
// N = (d, kw, o) over the two g rows oh + d (80 = 5 tiles), so
//     C[(r, i)][(d, kw, o)] += sum_q XC[i][oh - PH + r][q - PW] * gN[o][oh + d][q - kw] (+ C * gD)
// holds the kernel row kh = r - d of output row oh + d: gW[o][i][kh][kw] = C[(kh, i)][(0, kw, o)] +
// C[(kh + 1, i)][(1, kw, o)] (the pairs r = K, d = 0 and r = 0, d = 1 are not taps). 15 MFMAs per
// k-step and operand part for two rows instead of 18, and 8 operand reads instead of 12. The input
// ring holds K + 3 rows (K + 1 in use, two being written for the next pair), the g rows are double
// buffered per pair, the next pair staged under this pair's MFMAs; an odd last row pairs with a
// zero row. Same products, summed in a different
// (fixed) order: within fp32 round-off of wgrad_mfma, deterministic.
template <int CIN, int COUT, int K>
struct Wm2Cfg {
    static constexpr int TW = 64;
    static constexpr int M = (K + 1) * CIN, N = 2 * K * COUT;
    static constexpr int MT = M / 16, NT = N / 16;
    static_assert(M % 16 == 0 && N % 16 == 0, "row-pair tiles fill the MFMA tiles exactly");
    static constexpr int XP = TW + 2;  // == 2 (mod 32): a kernel row's channels on banks 2i + k
    static constexpr int SLOTS = 8;    // K + 3 <= 8: slot = input row & 7
    static_assert(K + 3 <= SLOTS, "input ring");
    // A: a 16-row tile holds two input rows in consecutive slots; SLOT == 16 (mod 32) puts the second
    // on the other 16 banks (and the ring's wrap, 7 slots back, is == 16 too)
    static constexpr int SLOT = CIN * XP + ((((2 * CIN) % 32 - CIN * XP) % 32) + 32) % 32;
    static constexpr int GP = 68;                      // B: channel o at 4o + {kw shifts} (mod 32)
    static constexpr int GROW = COUT * GP + ((((2 - COUT * GP) % 32) + 32) % 32);  // == 2 (mod 32):
    // the tile straddling d = 0 / 1 reads words 4o + {0, 1} and GROW + 4o + {4, 5}: distinct banks
    static constexpr int C_OFF = SLOTS * SLOT;         // c ring after the xc ring
    static constexpr int G_OFF = 2 * C_OFF;
    static constexpr int GPART = 2 * GROW;             // {gN rows d = 0, 1} then {gD rows}
    static constexpr int GBUF = 2 * GPART;
    static constexpr int STAGE = G_OFF + 2 * GBUF;
    static constexpr int TILE = MT * NT * 256;         // one wave's accumulators
    static constexpr int RED = 2 * TILE;               // waves 0 / 1 store, 2 / 3 add
    static constexpr int LDS = STAGE > RED ? STAGE : RED;
    static constexpr int CPW = (CIN + 3) / 4, OPW = COUT / 4;
    static_assert(SLOT % 32 == 16 && XP % 32 == 2 && GP % 32 == 4 && GROW % 32 == 2, "bank layout");
    static_assert(COUT % 4 == 0 && CIN % 4 == 0, "channels staged four per pass");
};

constexpr int kWm2Waves = 3;  // waves per SIMD asked of the compiler (wgrad_mfma2)
template <int CIN, int COUT, int K, int MODE, bool GP = false>
__global__ __launch_bounds__(kT) __attribute__((amdgpu_waves_per_eu(kWm2Waves, 8))) void wgrad_mfma2(
    LayerDev d, BwdArgs a, float* part, int nstrip, int nseg, int seg_rows) {
    using C = Wm2Cfg<CIN, COUT, K>;
    __shared__ __attribute__((aligned(16))) float lds[C::LDS];
    const nconv_layer& L = d.L;
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    int blk = blockIdx.x;
    const int strip = blk % nstrip;
    blk /= nstrip;
    const int seg = blk % nseg, b = blk / nseg;
    const int ow0 = strip * C::TW;
    const int r0 = seg * seg_rows, r1 = min(L.Ho, r0 + seg_rows);

    const int kq = lane >> 4, ml = lane & 15;
    int a_r[C::MT], a_ik[C::MT], b_off[C::NT];
#pragma unroll
    for (int t = 0; t < C::MT; ++t) {
        const int m = 16 * t + ml;
        a_r[t] = m / CIN;
        a_ik[t] = (m % CIN) * C::XP + kq;
    }
#pragma unroll
    for (int u = 0; u < C::NT; ++u) {
        const int n = 16 * u + ml, dd = n / (K * COUT), rem = n % (K * COUT);
        b_off[u] = dd * C::GROW + (rem % COUT) * C::GP + (K - 1) - rem / COUT + kq;
    }

    // ---- staging (two rows per pair; one row's loads in flight at a time, see the loop) ----
    float px[1][C::CPW], pc[1][C::CPW];
    const int iw_in = ow0 - L.PW + lane;
    // input row ih (valid: a row of this pair; else zeros, so no value of another segment enters)
    auto load_in = [&](int j, int ih, bool valid) {
#pragma unroll
        for (int kk = 0; kk < C::CPW; ++kk) {
            const int i = w + 4 * kk;
            px[j][kk] = pc[j][kk] = 0.f;
            if (valid) load_px<MODE>(d, chan_src<MODE>(d, b, i), ih, iw_in, px[j][kk], pc[j][kk]);
        }
    };
    auto store_in = [&](int j, int ih) {
        const int slot = ih & (C::SLOTS - 1);
#pragma unroll
        for (int kk = 0; kk < C::CPW; ++kk) {
            const int i = w + 4 * kk;
            const float cv = (MODE == NCONV_LOAD_THRESH) ? (px[j][kk] > L.thresh ? 1.0f : 0.0f) : pc[j][kk];
            lds[slot * C::SLOT + i * C::XP + lane] = px[j][kk] * cv;
            lds[C::C_OFF + slot * C::SLOT + i * C::XP + lane] = cv;
        }
    };
    using GS = GRowStager<COUT, K, C::GP, GP, false>;
    GS gs;
    gs.init(L, a, b, w, lane, ow0);
    // g row d of a pair into buffer buf: {gN rows d = 0, 1} then {gD rows}; a row past the segment
    // is not valid (zeros, and nothing added to the bias / normaliser sums)
    auto grow = [&](int buf, int dr) { return lds + C::G_OFF + buf * C::GBUF + dr * C::GROW; };

    f4acc acc[C::MT][C::NT];
#pragma unroll
    for (int t = 0; t < C::MT; ++t)
#pragma unroll
        for (int u = 0; u < C::NT; ++u) acc[t][u] = (f4acc){0.f, 0.f, 0.f, 0.f};

    // The next pair's rows are staged DURING this pair's MFMAs, one row (input + g) per half of the
    // k-steps: its input row goes to a ring slot this pair does not read (slots ih + 6, ih + 7 of
    // the 8), its g row to the other buffer (whose last reader, the previous pair, is behind the
    // barrier), so only one row's loads are ever in flight and one barrier per pair suffices.
    if (r0 < r1) {
        for (int r = 0; r <= K; ++r) {  // prologue: the first pair's K + 1 input rows and its g rows
            load_in(0, r0 - L.PH + r, r < K || r0 + 1 < r1);
            store_in(0, r0 - L.PH + r);
        }
        for (int j = 0; j < 2; ++j) {
            gs.load(L, a, r0 + j, j == 0 || r0 + 1 < r1);
            gs.store(L, a, grow(0, j), C::GPART, r0 + j, j == 0 || r0 + 1 < r1);
        }
    }
    __syncthreads();
#pragma unroll 1
    for (int oh = r0; oh < r1; oh += 2) {
        const int buf = ((oh - r0) >> 1) & 1;
        const int nx = oh + 2;  // the next pair (none past r1: its staging is skipped)
        const bool more = nx < r1;
        int ax[C::MT], bn[C::NT];
#pragma unroll
        for (int t = 0; t < C::MT; ++t) ax[t] = ((oh - L.PH + a_r[t]) & (C::SLOTS - 1)) * C::SLOT + a_ik[t];
#pragma unroll
        for (int u = 0; u < C::NT; ++u) bn[u] = C::G_OFF + buf * C::GBUF + b_off[u];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            if (more) {  // next pair's row j: input row r = K - 1 + j, g row d = j
                load_in(0, nx - L.PH + K - 1 + j, j == 0 || nx + 1 < r1);
                gs.load(L, a, nx + j, j == 0 || nx + 1 < r1);
            }
#pragma unroll
            for (int s = 2 * j; s < 2 * j + 2; ++s) {
                const int q0 = 16 * w + 4 * s;
#pragma unroll
                for (int pt = 0; pt < 2; ++pt) {  // {x*c, gN} then {c, gD}
                    float va[C::MT], vb[C::NT];
#pragma unroll
                    for (int t = 0; t < C::MT; ++t) va[t] = lds[ax[t] + pt * C::C_OFF + q0];
#pragma unroll
                    for (int u = 0; u < C::NT; ++u) vb[u] = lds[bn[u] + pt * C::GPART + q0];
#pragma unroll
                    for (int t = 0; t < C::MT; ++t)
#pragma unroll
                        for (int u = 0; u < C::NT; ++u)
                            acc[t][u] = __builtin_amdgcn_mfma_f32_16x16x4f32(va[t], vb[u], acc[t][u], 0, 0, 0);
                    __builtin_amdgcn_sched_barrier(0);  // (operand reads of the next step not hoisted above)
                }
            }
            if (more) {
                store_in(0, nx - L.PH + K - 1 + j);
                gs.store(L, a, grow(buf ^ 1, j), C::GPART, nx + j, j == 0 || nx + 1 < r1);
            }
        }
        __syncthreads();
    }

    // ---- the four waves' tiles summed in a fixed order ((w0 + w2) + (w1 + w3)), then each weight
    //      as its two row-pair terms: gW[o][i][kh][kw] = C[(kh, i)][(0, kw, o)] + C[(kh+1, i)][(1, kw, o)]
    constexpr int NW = COUT * CIN * K * K;
    float* out = part + (size_t)blockIdx.x * (NW + 2 * COUT);
    __syncthreads();
    float* red = lds + (w & 1) * C::TILE;
    if (w < 2) {
#pragma unroll
        for (int t = 0; t < C::MT; ++t)
#pragma unroll
            for (int u = 0; u < C::NT; ++u)
#pragma unroll
                for (int r = 0; r < 4; ++r) red[(t * C::NT + u) * 256 + r * 64 + lane] = acc[t][u][r];
    }
    __syncthreads();
    if (w >= 2) {
#pragma unroll
        for (int t = 0; t < C::MT; ++t)
#pragma unroll
            for (int u = 0; u < C::NT; ++u)
#pragma unroll
                for (int r = 0; r < 4; ++r) red[(t * C::NT + u) * 256 + r * 64 + lane] += acc[t][u][r];
    }
    __syncthreads();
    auto at = [&](int m, int n) {  // the summed C[m][n] (MFMA 16x16 output layout)
        const int t = m >> 4, mm = m & 15, u = n >> 4;
        const int idx = (t * C::NT + u) * 256 + (mm & 3) * 64 + (mm >> 2) * 16 + (n & 15);
        return lds[idx] + lds[C::TILE + idx];
    };
    for (int f = tid; f < NW; f += kT) {  // o fastest: a wave's reads spread over the LDS banks
        const int o = f % COUT, kw = (f / COUT) % K, kh = (f / (COUT * K)) % K, i = f / (COUT * K * K);
        out[((o * CIN + i) * K + kh) * K + kw] =
            at(kh * CIN + i, kw * COUT + o) + at((kh + 1) * CIN + i, K * COUT + kw * COUT + o);
    }
    gs.finish(a, out + NW);
}

// ---- launchers --------------------------------------------------------------------------------------
// Grid: 64-wide q strips (q = ow + kw spans Wo + K - 1 columns) x row segments x images,
// at most `target` workgroups: kMfmaRounds resident rounds of the instantiation (CUs x blocks
// per CU x rounds; a third, nearly empty round once cost nconv2's weight gradient a third of its
// time). One round (longer row segments: less per-block prologue, fewer partial rows) for the
// weight gradients that share the CUs with the input-gradient chain, two for the tail's (T7), which
// starts the side stream: graphed training step 2.104 -> 2.064 ms same box (one round everywhere
// 2.093, the tail alone at one round 2.137; profiles/r6_ab_wgrad_rounds.log). The workspace is
// sized for the larger round count at the largest possible occupancy (kMfmaRoundsMax).
constexpr int kMfmaRounds = 1, kMfmaT7Rounds = 2, kMfmaMaxPerCu = 4;
constexpr int kMfmaRoundsMax = kMfmaT7Rounds > kMfmaRounds ? kMfmaT7Rounds : kMfmaRounds;
struct WmGrid {
    int nstrip, nseg, seg_rows;
    size_t nblk;
};
static WmGrid wm_grid(const nconv_layer& L, int target) {
    WmGrid g;
    g.nstrip = (L.Wo + L.KW - 1 + 63) / 64;
    const int per_img = g.nstrip * L.B;
    int nseg = target / per_img;  // floor: never more blocks than the target (nseg >= 1 below)
    nseg = nseg < 1 ? 1 : (nseg > L.Ho ? L.Ho : nseg);
    g.seg_rows = (L.Ho + nseg - 1) / nseg;
    if (g.seg_rows < 1) g.seg_rows = 1;
    g.nseg = (L.Ho + g.seg_rows - 1) / g.seg_rows;
    if (g.nseg < 1) g.nseg = 1;
    g.nblk = (size_t)g.nstrip * g.nseg * L.B;
    return g;
}

size_t wgrad_mfma_max_blocks(const nconv_layer& L) {  // the workspace bound (every variant)
    return wm_grid(L, kMfmaRoundsMax * kMfmaMaxPerCu * dev_cus()).nblk;
}

template <typename Kern>
static int launch_wm(Kern kern, int rounds, const LayerDev& d, const BwdArgs& a, float* part, hipStream_t st) {
    const int per_cu = dev_occupancy((const void*)kern, kT, 0);
    const int resident = dev_cus() * (per_cu < kMfmaMaxPerCu ? per_cu : kMfmaMaxPerCu);
    const WmGrid g = wm_grid(d.L, rounds * resident);
    hipLaunchKernelGGL(kern, dim3(g.nblk), dim3(kT), 0, st, d, a, part, g.nstrip, g.nseg, g.seg_rows);
    return (int)g.nblk;
}

template <int CIN, int COUT, int K, int MODE, bool GP, bool T7>
int go_wgrad_mfma(const LayerDev& d, const BwdArgs& a, float* part, hipStream_t st) {
    if constexpr (CIN == 8 && COUT == 8 && K == 5) {  // the row-pair form fills its MFMA tiles
        static_assert(!T7, "the fused nconv7 backward belongs to nconv6 (16 -> 8 3x3)");
        return launch_wm(wgrad_mfma2<CIN, COUT, K, MODE, GP>, kMfmaRounds, d, a, part, st);
    } else {
        static_assert(!GP, "pooled-gradient routing: the 8 -> 8 5x5 layers");
        if constexpr (T7)
            if (a.t7gco) return launch_wm(wgrad_mfma<CIN, COUT, K, MODE, false, true>, kMfmaT7Rounds, d, a, part, st);
        return launch_wm(wgrad_mfma<CIN, COUT, K, MODE, T7>, T7 ? kMfmaT7Rounds : kMfmaRounds, d, a, part, st);
    }
}

#define NCONV_GO_WGRAD_MFMA(CIN, COUT, K, MODE, GP, T7) \
    template int go_wgrad_mfma<CIN, COUT, K, MODE, GP, T7>(const LayerDev&, const BwdArgs&, float*, hipStream_t);
NCONV_GO_WGRAD_MFMA(8, 8, 5, NCONV_LOAD_PLAIN, false, false)
NCONV_GO_WGRAD_MFMA(8, 8, 5, NCONV_LOAD_PLAIN, true, false)
NCONV_GO_WGRAD_MFMA(8, 8, 5, NCONV_LOAD_POOL2, false, false)
NCONV_GO_WGRAD_MFMA(16, 8, 3, NCONV_LOAD_UPCAT_SKIP_FIRST, false, false)
NCONV_GO_WGRAD_MFMA(16, 8, 3, NCONV_LOAD_UPCAT_UP_FIRST, false, false)
NCONV_GO_WGRAD_MFMA(16, 8, 3, NCONV_LOAD_UPCAT_UP_FIRST, false, true)
#undef NCONV_GO_WGRAD_MFMA

}  // namespace nconv
