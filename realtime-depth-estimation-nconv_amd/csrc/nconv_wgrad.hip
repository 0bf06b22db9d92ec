// nconv_wgrad.hip — exact-fp32 weight-gradient ("wgrad") kernels of the NConv backward on the vector
// ALUs, and the fixed-order reduction every weight-gradient kernel ends in (the math:
// nconv_bwd.hip's header).
#include "nconv_internal.h"
#include "nconv_route.h"

namespace nconv {

constexpr int kT = 256;

// ---- wgrad: tiled partial sums, stride 1 ------------------------------------------------------------
// A thread owns one (o, i) weight pair with all K*K taps in registers and a subset ("sub") of each
// 4 x 64 output tile: rows, or for small Cin*Cout also column segments, so all 256 threads work
// for every layer shape. Per output pixel it reads g = {gN, gD} once and, for each kernel row, one
// new input {x*c, c} into a sliding window: K+1 LDS reads per K*K packed FMAs
// {sum x*c*gN, sum c*gD} += {x*c, c} * {gN, gD}.
constexpr int pow2ceil(int n) {
    int p = 1;
    while (p < n) p <<= 1;
    return p;
}

// One kernel row of the weight-gradient correlation over SEGW output columns:
// acc[kw] += in[c + kw] * g[c]  ({x*c, c} * {gN, gD} elementwise). Circular window: input column
// c lives in slot c % K; stepping K columns at a time keeps every slot index a compile-time
// constant, so the window never moves between registers.
template <int K, int SEGW>
__device__ __forceinline__ void wgrad_row(const f2* ir, const f2* gr, f2 (&acc)[K]) {
    f2 win[K];
#pragma unroll
    for (int kw = 0; kw < K - 1; ++kw) win[kw] = ir[kw];
    constexpr int NSTEP = SEGW / K, REM = SEGW % K;
#pragma unroll 2
    for (int st = 0; st < NSTEP; ++st) {
        const int cc = st * K;
#pragma unroll
        for (int j = 0; j < K; ++j) {
            const f2 g = gr[cc + j];
            win[(j + K - 1) % K] = ir[cc + j + K - 1];
#pragma unroll
            for (int kw = 0; kw < K; ++kw) acc[kw] = __builtin_elementwise_fma(win[(j + kw) % K], g, acc[kw]);
        }
    }
#pragma unroll
    for (int j = 0; j < REM; ++j) {
        const int cc = NSTEP * K;
        const f2 g = gr[cc + j];
        win[(j + K - 1) % K] = ir[cc + j + K - 1];
#pragma unroll
        for (int kw = 0; kw < K; ++kw) acc[kw] = __builtin_elementwise_fma(win[(j + kw) % K], g, acc[kw]);
    }
}

template <int CIN, int COUT, int K>
struct WgCfg {
    static constexpr int TH = 4, TW = 64;  // TH*TW == kT: one output pixel per thread while staging
    static constexpr int IHT = TH + K - 1, IHTP = (IHT + 3) / 4 * 4, IWT = TW + K - 1;
    // plane strides = 1 (mod 32) f2 so that the distinct channel planes a wave reads hit
    // different bank pairs (bank = dword % 64).
    static constexpr int IPL = ((IHTP * IWT + 31) / 32) * 32 + 1;
    static constexpr int GPL = TH * TW + 1;
    static constexpr int CW = CIN < 8 ? CIN : 8;  // input channels staged per chunk
    static_assert(CIN % CW == 0, "input channel chunking");
    static constexpr int NCH = CIN / CW;
    static constexpr int NCB = COUT * CW;  // (o, i) pairs of one chunk
    static constexpr int NCBP = pow2ceil(NCB);
    static_assert(NCBP <= kT, "wgrad_tiled: Cout*min(Cin,8) must be <= 256");
    static_assert(K <= 7, "wgrad_tiled: kernel rows dispatched through a switch of 7 cases");
    static constexpr int NSUB = kT / NCBP;
    static constexpr int NSEG = NSUB > TH ? NSUB / TH : 1;  // column segments per row
    static constexpr int SEGW = TW / NSEG;
    static constexpr int LDS_F2 = CW * IPL + COUT * GPL;
};

template <int CIN, int COUT, int K, int MODE>
__global__ __launch_bounds__(kT) void wgrad_tiled(LayerDev d, BwdArgs a, float* part, int ntile_w,
                                                  int ntile_h) {
    using C = WgCfg<CIN, COUT, K>;
    extern __shared__ __attribute__((aligned(16))) f2 smem[];
    f2* sin = smem;
    f2* sg = smem + C::CW * C::IPL;
    const nconv_layer& L = d.L;
    const int tid = threadIdx.x;
    const int ntiles = ntile_w * ntile_h * L.B;
    const int cb = tid % C::NCBP, sub = tid / C::NCBP;
    const bool active = cb < C::NCB;
    const int il = active ? cb % C::CW : 0, o = active ? cb / C::CW : 0;
    // rows / column segment of this thread's sub
    const int r_first = (C::NSUB > C::TH) ? sub % C::TH : sub;
    const int r_step = (C::NSUB > C::TH) ? C::TH : C::NSUB;
    const int c_first = (C::NSUB > C::TH) ? (sub / C::TH) * C::SEGW : 0;

    f2 acc[C::NCH][K][K];
#pragma unroll
    for (int ch = 0; ch < C::NCH; ++ch)
#pragma unroll
        for (int kh = 0; kh < K; ++kh)
#pragma unroll
            for (int kw = 0; kw < K; ++kw) acc[ch][kh][kw] = (f2){0.f, 0.f};
    float gb_acc[COUT], gs_acc[COUT];
#pragma unroll
    for (int oo = 0; oo < COUT; ++oo) gb_acc[oo] = gs_acc[oo] = 0.f;

    // a contiguous run of row-major tiles per block: neighbouring tiles' halos hit the same L2
    const int per_blk = (ntiles + gridDim.x - 1) / gridDim.x;
    const int t_end = min(ntiles, ((int)blockIdx.x + 1) * per_blk);
    for (int t = blockIdx.x * per_blk; t < t_end; ++t) {
        const int tw = t % ntile_w, th = (t / ntile_w) % ntile_h, b = t / (ntile_w * ntile_h);
        const int oh0 = th * C::TH, ow0 = tw * C::TW;
        const int ih0 = oh0 - L.PH, iw0 = ow0 - L.PW;
        __syncthreads();
        {   // g plane: one output pixel per thread per channel; loads clamped and issued up front
            const int r = tid / C::TW, col = tid % C::TW;
            const int oh = oh0 + r, ow = ow0 + col;
            const bool in = (oh < L.Ho) && (ow < L.Wo);
            const int ohc = oh < L.Ho ? oh : L.Ho - 1, owc = ow < L.Wo ? ow : L.Wo - 1;
#pragma unroll
            for (int oo = 0; oo < COUT; ++oo) {
                const size_t gi = plane_idx(b, oo, COUT, L.Ho, L.Wo, ohc, owc);
                const float gy = a.gy[gi], co = a.co[gi], yv = a.y[gi];
                const float gco = a.gco ? a.gco[gi] : 0.f;
                float gN, gD;
                nconv_grad_nd(gy, gco, yv, co, L.eps, L.bias[oo], L.wsum[oo], gN, gD);
                gb_acc[oo] += in ? gy : 0.f;
                gs_acc[oo] = in ? fmaf(gco, co, gs_acc[oo]) : gs_acc[oo];
                sg[oo * C::GPL + tid] = in ? (f2){gN, gD} : (f2){0.f, 0.f};
            }
        }
#pragma unroll
        for (int ch = 0; ch < C::NCH; ++ch) {
            if (ch) __syncthreads();
            for (int ci = 0; ci < C::CW; ++ci)
                stage_plane<C::IHT, C::IWT, C::IWT>(d, chan_src<MODE>(d, b, ch * C::CW + ci), sin + ci * C::IPL, ih0,
                                                    iw0, tid);
            __syncthreads();
            if (active) {
                for (int r = r_first; r < C::TH; r += r_step) {
                    const f2* gr = sg + o * C::GPL + r * C::TW + c_first;
                    // kernel rows one at a time (a runtime loop over a compile-time switch keeps
                    // acc statically indexed without letting the scheduler hoist every row's
                    // LDS reads into registers at once)
#pragma unroll 1
                    for (int kh = 0; kh < K; ++kh) {
                        const f2* ir = sin + il * C::IPL + (r + kh) * C::IWT + c_first;
                        switch (kh) {
#define NCONV_WG_ROW(KH) \
    case KH:             \
        if constexpr (KH < K) wgrad_row<K, C::SEGW>(ir, gr, acc[ch][KH]); \
        break;
                            NCONV_WG_ROW(0)
                            NCONV_WG_ROW(1)
                            NCONV_WG_ROW(2)
                            NCONV_WG_ROW(3)
                            NCONV_WG_ROW(4)
                            NCONV_WG_ROW(5)
                            NCONV_WG_ROW(6)
#undef NCONV_WG_ROW
                        }
                    }
                }
            }
        }
    }

    // ---- combine the subs in a fixed order, then the gb / gs sums; write the partial row ----
    // partial[blk] = { gW-partial[COUT*CIN*K*K], sum gy[COUT], sum gco*cout[COUT] }
    constexpr int NW = COUT * CIN * K * K;
    float* out = part + (size_t)blockIdx.x * (NW + 2 * COUT);
    float* red = reinterpret_cast<float*>(smem);
    __syncthreads();
    if (active) {
#pragma unroll
        for (int ch = 0; ch < C::NCH; ++ch) {
            const int i = ch * C::CW + il;
#pragma unroll
            for (int kh = 0; kh < K; ++kh)
#pragma unroll
                for (int kw = 0; kw < K; ++kw)
                    red[sub * NW + ((o * CIN + i) * K + kh) * K + kw] = acc[ch][kh][kw].x + acc[ch][kh][kw].y;
        }
    }
    __syncthreads();
    for (int w = tid; w < NW; w += kT) {
        float sum = 0.f;
        for (int sb = 0; sb < C::NSUB; ++sb) sum += red[sb * NW + w];
        out[w] = sum;
    }
    __syncthreads();
#pragma unroll
    for (int oo = 0; oo < COUT; ++oo) {
        red[oo * kT + tid] = gb_acc[oo];
        red[(COUT + oo) * kT + tid] = gs_acc[oo];
    }
    __syncthreads();
    if (tid < 2 * COUT) {
        float sum = 0.f;
        for (int k = 0; k < kT; ++k) sum += red[tid * kT + k];
        out[NW + tid] = sum;
    }
}

// ---- wgrad: generic partial sums (any stride / dilation / groups) -----------------------------------
// grid = (nchunk, n_weight + 2*Cout): blockIdx.y selects a weight element (or a gb / gs sum),
// blockIdx.x a contiguous chunk of the (b, oh, ow) reduction domain.
template <int MODE>
__global__ __launch_bounds__(kT) void wgrad_generic(LayerDev d, BwdArgs a, float* part, int nchunk) {
    const nconv_layer& L = d.L;
    const int cpg_in = L.Cin / L.groups, cpg_out = L.Cout / L.groups;
    const int fan = cpg_in * L.KH * L.KW;
    const int nw = L.Cout * fan;
    const int widx = blockIdx.y;
    const size_t np = (size_t)L.B * L.Ho * L.Wo;
    const size_t per = (np + nchunk - 1) / nchunk;
    const size_t p0 = (size_t)blockIdx.x * per, p1 = p0 + per < np ? p0 + per : np;
    int o, cl = 0, kh = 0, kw = 0, kind;  // kind 0: weight, 1: gb, 2: gs
    if (widx < nw) {
        kind = 0;
        o = widx / fan;
        int r = widx - o * fan;
        cl = r / (L.KH * L.KW);
        r -= cl * L.KH * L.KW;
        kh = r / L.KW;
        kw = r - kh * L.KW;
    } else if (widx < nw + L.Cout) {
        kind = 1;
        o = widx - nw;
    } else {
        kind = 2;
        o = widx - nw - L.Cout;
    }
    const int ci = (o / cpg_out) * cpg_in + cl;
    const float bo = L.bias[o], so = L.wsum[o];
    float acc = 0.f;
    for (size_t p = p0 + threadIdx.x; p < p1; p += kT) {
        const int ow = (int)(p % L.Wo), oh = (int)((p / L.Wo) % L.Ho), b = (int)(p / ((size_t)L.Wo * L.Ho));
        const size_t i = plane_idx(b, o, L.Cout, L.Ho, L.Wo, oh, ow);
        const float gy = a.gy[i], gco = a.gco ? a.gco[i] : 0.f;
        if (kind == 1) { acc += gy; continue; }
        if (kind == 2) { acc = fmaf(gco, a.co[i], acc); continue; }
        const int ih = oh * L.SH - L.PH + kh * L.DH, iw = ow * L.SW - L.PW + kw * L.DW;
        if ((unsigned)ih >= (unsigned)L.H || (unsigned)iw >= (unsigned)L.W) continue;
        float gN, gD, x, c;
        nconv_grad_nd(gy, gco, a.y[i], a.co[i], L.eps, bo, so, gN, gD);
        load_xc<MODE>(d, b, ci, ih, iw, x, c);
        acc = fmaf(x * c, gN, acc);
        acc = fmaf(c, gD, acc);
    }
    __shared__ float red[kT];
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int s = kT / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) part[(size_t)blockIdx.x * (nw + 2 * L.Cout) + widx] = red[0];
}

// ---- wgrad: fixed-order reduction of the per-block partials ----------------------------------------
// Stage 1: sub[y][e] = sum of part[k][e] over the y-th of kReduceSplit contiguous slices of the
// partial rows, for every entry e of a row (weights, sum gy, sum gco*cout). A 256-thread block owns
// 64 consecutive entries of one slice; its 4 waves sum interleaved rows (coalesced 256-B rows,
// 8 independent loads in flight per lane) and combine the 4 subtotals in LDS in a fixed order.
// Stage 2 (wgrad_finish) adds the kReduceSplit slice sums in order — deterministic, no atomics.

// Both stages take a table of up to kMaxRedJobs layers (nconv_wgrad_reduce: every layer of a
// backward pass in two launches instead of two per layer); a block finds its layer by a
// wave-uniform scan of the table's first-block offsets.
struct RedTable {
    RedJob j[kMaxRedJobs];
    int x0[kMaxRedJobs + 1];  // first stage-1 block (64 entries of a row) of each job
    int f0[kMaxRedJobs + 1];  // first stage-2 block of each job
    int n;
};

__device__ __forceinline__ int red_job(const int* first, int n, int blk) {
    int k = 0;
    while (k + 1 < n && blk >= first[k + 1]) ++k;
    return k;
}

// A flat job's chunk sum (nconv_wgrad_reduce_ex): chunk c of kSumChunks contiguous chunks of the
// vector, lane-strided partial sums, then a fixed-order LDS tree.
__device__ __forceinline__ float block_tree_sum(float* red, float s) {
    red[threadIdx.x] = s;
    __syncthreads();
#pragma unroll
    for (int h = kT / 2; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
        __syncthreads();
    }
    return red[0];
}

__global__ __launch_bounds__(kT) void wgrad_reduce_sum(const RedTable T) {
    __shared__ float red[kT];
    const int k = red_job(T.x0, T.n, blockIdx.x);
    const RedJob& J = T.j[k];
    if (J.flat) {
        const int c = (blockIdx.x - T.x0[k]) * kReduceSplit + blockIdx.y;
        const long long n = J.nblk, per = (n + kSumChunks - 1) / kSumChunks;
        const long long e0 = c * per, e1 = e0 + per < n ? e0 + per : n;
        float s = 0.f;
        for (long long e = e0 + threadIdx.x; e < e1; e += kT) s += J.part[e];
        const float t = block_tree_sum(red, s);
        if (threadIdx.x == 0) J.sub[c] = t;
        return;
    }
    const int stride = J.nw + 2 * J.cout, nblk = J.nblk;
    const float* part = J.part;
    float* sub = const_cast<float*>(J.part) + (size_t)nblk * stride;
    const int lane = threadIdx.x & 63, grp = threadIdx.x >> 6;
    const int e = (blockIdx.x - T.x0[k]) * 64 + lane;
    const int per = (nblk + kReduceSplit - 1) / kReduceSplit;
    const int k0 = blockIdx.y * per, k1 = min(nblk, k0 + per);
    float s = 0.f;
    if (e < stride) {
        int r = k0 + grp;
        for (; r + 28 < k1; r += 32) {
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = part[(size_t)(r + 4 * u) * stride + e];
#pragma unroll
            for (int u = 0; u < 8; ++u) s += v[u];
        }
        for (; r < k1; r += 4) s += part[(size_t)r * stride + e];
    }
    red[threadIdx.x] = s;
    __syncthreads();
    if (grp == 0 && e < stride)
        sub[(size_t)blockIdx.y * stride + e] = ((red[lane] + red[64 + lane]) + red[128 + lane]) + red[192 + lane];
}

// Stage 2: tot = sum of the slice sums; gW[w] = tot[w] + gs[o(w)] with gs = -(sum gco*cout)/s
// (d cout / d s, cout = D/s), gb = sum gy.
__device__ __forceinline__ float slice_total(const float* sub, int stride, int e) {
    float t = 0.f;
#pragma unroll
    for (int y = 0; y < kReduceSplit; ++y) t += sub[(size_t)y * stride + e];
    return t;
}

__global__ __launch_bounds__(kT) void wgrad_finish(const RedTable T) {
    __shared__ float red[kT];
    const int k = red_job(T.f0, T.n, blockIdx.x);
    const RedJob& J = T.j[k];
    if (J.flat) {  // the kSumChunks chunk sums: kSumChunks / kT per thread in order, then the tree
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < kSumChunks / kT; ++i) s += J.sub[threadIdx.x * (kSumChunks / kT) + i];
        const float t = block_tree_sum(red, s);
        if (threadIdx.x == 0) J.gb[0] = t;
        return;
    }
    const int nw = J.nw, cout = J.cout, stride = nw + 2 * cout;
    const float* sub = J.part + (size_t)J.nblk * stride;
    const int w = (blockIdx.x - T.f0[k]) * kT + threadIdx.x;
    if (w < nw) {
        const int o = w / J.fan;
        if (J.gw) J.gw[w] = slice_total(sub, stride, w) + (-slice_total(sub, stride, nw + cout + o) / J.wsum[o]);
    } else if (w < nw + cout && J.gb) {
        J.gb[w - nw] = slice_total(sub, stride, w);
    }
}

int launch_wgrad_reduce_multi(int n, const RedJob* jobs, hipStream_t st, const char** why) {
    if (n < 1 || n > kMaxRedJobs) {
        *why = "between 1 and 16 layers per reduction";
        return -22;
    }
    RedTable T;
    T.n = n;
    T.x0[0] = T.f0[0] = 0;
    static_assert(kSumChunks % kReduceSplit == 0 && kSumChunks % kT == 0, "flat chunks");
    for (int k = 0; k < n; ++k) {
        T.j[k] = jobs[k];
        const int stride = jobs[k].nw + 2 * jobs[k].cout;
        T.x0[k + 1] = T.x0[k] + (jobs[k].flat ? kSumChunks / kReduceSplit : (stride + 63) / 64);
        T.f0[k + 1] = T.f0[k] + (jobs[k].flat ? 1 : (jobs[k].nw + jobs[k].cout + kT - 1) / kT);
    }
    for (int k = n + 1; k <= kMaxRedJobs; ++k) T.x0[k] = T.f0[k] = 0;
    hipLaunchKernelGGL(wgrad_reduce_sum, dim3(T.x0[n], kReduceSplit), dim3(kT), 0, st, T);
    hipLaunchKernelGGL(wgrad_finish, dim3(T.f0[n]), dim3(kT), 0, st, T);
    return launch_status(why);
}

// part: nblk partial rows followed by kReduceSplit rows of slice sums (see bwd_layout);
// with a.defer the rows stay for a later nconv_wgrad_reduce over every layer of the pass
int launch_wgrad_reduce(const BwdArgs& a, const float* part, int nblk, int nw, int cout, int fan,
                        const float* wsum, hipStream_t st, const char** why) {
    if (a.defer) {
        *a.nparts = nblk;
        return 0;
    }
    const RedJob J{part, wsum, a.gw, a.gb, nblk, nw, cout, fan};
    return launch_wgrad_reduce_multi(1, &J, st, why);
}

// ---- launchers --------------------------------------------------------------------------------------
template <int CIN, int COUT, int K, int MODE>
int go_wgrad_tiled(const LayerDev& d, const BwdArgs& a, float* part, int max_blocks, hipStream_t st) {
    using W = WgCfg<CIN, COUT, K>;
    const nconv_layer& L = d.L;
    const int ntw = (L.Wo + W::TW - 1) / W::TW, nth = (L.Ho + W::TH - 1) / W::TH;
    size_t lds = (size_t)W::LDS_F2 * sizeof(f2);
    size_t red = (size_t)2 * COUT * kT * sizeof(float);
    const size_t red2 = (size_t)W::NSUB * COUT * CIN * K * K * sizeof(float);
    if (red2 > red) red = red2;
    if (red > lds) lds = red;
    // blocks walk runs of tiles: launch at most the resident count (CUs x blocks per CU), so
    // there is no second, partial round (nconv1's 13.4 k tiles: 768 resident at 3 waves/SIMD)
    const int resident = dev_cus() * dev_occupancy((const void*)wgrad_tiled<CIN, COUT, K, MODE>, kT, lds);
    const int nblk = max_blocks < resident ? max_blocks : resident;
    hipLaunchKernelGGL((wgrad_tiled<CIN, COUT, K, MODE>), dim3(nblk), dim3(kT), lds, st, d, a, part, ntw, nth);
    return nblk;
}

template int go_wgrad_tiled<1, 8, 5, NCONV_LOAD_THRESH>(const LayerDev&, const BwdArgs&, float*, int, hipStream_t);
template int go_wgrad_tiled<8, 1, 1, NCONV_LOAD_PLAIN>(const LayerDev&, const BwdArgs&, float*, int, hipStream_t);

int launch_wgrad_generic(const LayerDev& d, const BwdArgs& a, float* part, int nchunk, hipStream_t st,
                         const char** why) {
    const nconv_layer& L = d.L;
    const dim3 g(nchunk, L.Cout * (L.Cin / L.groups) * L.KH * L.KW + 2 * L.Cout);
    switch (L.load_mode) {
#define NCONV_WG_GENERIC(M) \
    case M: hipLaunchKernelGGL(wgrad_generic<M>, g, dim3(kT), 0, st, d, a, part, nchunk); return 0;
        NCONV_WG_GENERIC(NCONV_LOAD_PLAIN)
        NCONV_WG_GENERIC(NCONV_LOAD_THRESH)
        NCONV_WG_GENERIC(NCONV_LOAD_POOL2)
        NCONV_WG_GENERIC(NCONV_LOAD_UPCAT_SKIP_FIRST)
        NCONV_WG_GENERIC(NCONV_LOAD_UPCAT_UP_FIRST)
#undef NCONV_WG_GENERIC
    }
    *why = "unknown load mode";
    return -22;
}

}  // namespace nconv
