// pose_align.hip — the relative camera pose between the current (target) frame and a neighbouring (source)
// frame from the target's sparse depth, by direct image alignment (Kerl, Sturm, Cremers, ICRA 2013; LSD-SLAM's
// tracker): the 6-DoF pose that minimises the intensity difference between the target frame at the depth
// samples and the source frame at their projections, by damped Gauss-Newton on SE(3). It produces the
// m = K_src . [R | t] that view_warp.hip, photo_ssim.hip and the training losses take as an input. The rule
// is stated operation by operation in include/nconv.h (nconv_pose_*).
//
//   pose_normal_eq   one workgroup of 256 threads per 16 x 64 tile of one image (warp_common.h's tile and
//                    thread map). Per sample (z > z_min && z <= z_max, its mask, its projection inside the
//                    source) and channel: the residual r = s - tgt, the 1 x 6 Jacobian J = dIu Ju + dIv Jv of
//                    the left perturbation, the Huber weight w; fp32, one rounding per operation, no
//                    contraction. u, v, valid, s, dIu and dIv are warp_common.h's, so they are
//                    nconv_view_warp's bit for bit. Per tile: the 28 fp32 sums (21 of the upper triangle of
//                    sum w J^T J, 6 of sum w J r, sum w r^2), a thread's rows in order, then wave_ops.h's
//                    wave_sum and waves_in_order, and the exact count. A wave without a sample skips the
//                    butterflies: its totals are the +0 they would have produced.
//   pose_update      one wave per image, all of it in double with a fixed order and no contraction: the tiles
//                    by image_tile_sums, A = H + damping diag(H), a square-root-free Cholesky (L D L^T: only
//                    + - x /, so numpy reproduces it bit for bit) of A delta = -b, the Cayley retraction
//                    R <- dR R, t <- dR t + nu on the double pose state kept in the workspace, the fp32 pose
//                    and m = K_src [R | t] rounded once, cost[it] and n[it].
//
// One Gauss-Newton iteration is these two launches. No atomics, no host synchronisation, no allocation:
// capturable, and the same bits on every run. Every load goes through a bounded buffer resource (an invalid
// pixel's loads are aimed at plane_io.h's kOOB); the partials are written at blockIdx.x < B * tiles, the
// update's outputs at b < B and it < history, both checked by the C boundary before the launch.
#include "warp_common.h"

namespace nconv {

namespace {

constexpr int kPS = kPoseSums;

// the workspace: the double pose state first (a caller initialises it there), the combined sums, the tiles
struct PoseWs {
    double* state;  // [B * 12]: [R | t] row-major
    double* sums;   // [B * kPS]: the image's sums as the last update combined them
    float* part;    // [B * tiles * kPS]
    int* cnt;       // [B * tiles]
};
__host__ __device__ PoseWs pose_ws(void* ws, int B, int tiles) {
    PoseWs p;
    p.state = (double*)ws;
    p.sums = p.state + (size_t)B * 12;
    p.part = (float*)(p.sums + (size_t)B * kPS);
    p.cnt = (int*)(p.part + (size_t)B * tiles * kPS);
    return p;
}

struct PoseCam {
    float fxs, fys;
    float p[3][4];
};

template <int C>
__global__ __launch_bounds__(kWT) void pose_normal_eq(PoseArgs pa, float* __restrict__ part, int* __restrict__ cnt) {
#pragma clang fp contract(off)
    __shared__ float red[kPS][kWT / 64];
    __shared__ int redc[kWT / 64];
    const WarpArgs& a = pa.w;
    const WarpTile t = warp_tile(a);
    const Camera cam = warp_camera(a, t.b);
    const Proj q = proj_of(a, t.b);
    PoseCam pc;
    {
        const float* ks = pa.k_src + (long long)t.b * pa.ksbs;
        const float* po = pa.pose + (long long)t.b * 12;
        pc.fxs = ks[0], pc.fys = ks[4];
#pragma unroll
        for (int k = 0; k < 12; ++k) pc.p[k / 4][k % 4] = po[k];
    }
    float acc[kPS];
#pragma unroll
    for (int k = 0; k < kPS; ++k) acc[k] = 0.f;
    int n = 0;
#pragma unroll
    for (int r = 0; r < kWRows; ++r) {
        const int i = t.i0 + r * (kWT / 64);
        const bool inside = i < a.H && t.j < a.W;
        const Geo g = warp_geometry(a, cam, q, t.b, i, t.j, inside);
        n += g.ok ? 1 : 0;
        if (!__any(g.ok)) continue;  // wave-uniform: no lane of this row has a sample, every term is +0
        // the point in the source camera's frame and the projection's derivative
        const __amdgpu_buffer_rsrc_t rd = plane_rsrc(a.depth.image<float>(t.b), view_bytes(a.H, a.depth.rs, a.W, 4));
        const float z = ld_f32(rd, g.ok ? (unsigned)((long long)i * a.depth.rs + t.j) * 4u : kOOB);
        float x, y;
        project(cam, i, t.j, z, x, y);
        const float Xp = warp_dot(pc.p[0], x, y, z), Yp = warp_dot(pc.p[1], x, y, z), Zp = warp_dot(pc.p[2], x, y, z);
        const float xn = Xp / Zp, yn = Yp / Zp, iz = 1.0f / Zp;
        const float xx = xn * xn, yy = yn * yn, xy = xn * yn;
        float Ju[6], Jv[6];
        Ju[0] = pc.fxs * iz;
        Ju[2] = -(pc.fxs * (xn * iz));
        Ju[3] = -(pc.fxs * xy);
        Ju[4] = pc.fxs * (1.0f + xx);
        Ju[5] = -(pc.fxs * yn);
        Jv[1] = pc.fys * iz;
        Jv[2] = -(pc.fys * (yn * iz));
        Jv[3] = -(pc.fys * (1.0f + yy));
        Jv[4] = pc.fys * xy;
        Jv[5] = pc.fys * xn;
        float term[kPS];
#pragma unroll
        for (int ch = 0; ch < C; ++ch) {
            const Sample p = warp_sample(a, g, t.b, ch);
            const float res = p.s - tgt_load(a, t.b, ch, i, t.j, g.ok);
            const float d0 = p.a01 - p.a00, d1 = p.a11 - p.a10;
            const float e0 = g.w0v * d0, e1 = g.wv * d1;
            const float dIu = e0 + e1;
            const float dIv = p.bot - p.top;
            float J[6];
            J[0] = dIu * Ju[0];
            J[1] = dIv * Jv[1];
#pragma unroll
            for (int k = 2; k < 6; ++k) {
                const float ju = dIu * Ju[k], jv = dIv * Jv[k];
                J[k] = ju + jv;
            }
            const float ar = fabsf(res);
            const float w = (pa.huber == 0.f || ar <= pa.huber) ? 1.0f : pa.huber / ar;
            int o = 0;
#pragma unroll
            for (int k = 0; k < 6; ++k) {
                const float wj = w * J[k];
#pragma unroll
                for (int l = k; l < 6; ++l, ++o) {
                    const float h = wj * J[l];
                    term[o] = ch == 0 ? h : term[o] + h;
                }
                const float bk = wj * res;
                term[21 + k] = ch == 0 ? bk : term[21 + k] + bk;
            }
            const float wr = w * res;
            const float e = wr * res;
            term[27] = ch == 0 ? e : term[27] + e;
        }
#pragma unroll
        for (int k = 0; k < kPS; ++k) acc[k] += g.ok ? term[k] : 0.f;
    }
    n = wave_sum(n);
    const int wave = threadIdx.x >> 6;
    if (n != 0) {  // wave-uniform
#pragma unroll
        for (int k = 0; k < kPS; ++k) acc[k] = wave_sum(acc[k]);
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < kPS; ++k) red[k][wave] = n != 0 ? acc[k] : 0.f;
        redc[wave] = n;
    }
    __syncthreads();
    if (threadIdx.x < kPS) part[(size_t)blockIdx.x * kPS + threadIdx.x] = waves_in_order(red[threadIdx.x]);
    if (threadIdx.x == 64) cnt[blockIdx.x] = waves_in_order(redc);
}

// One wave per image. apply == 0: only cost[it] and n[it] (the cost at the pose already reached).
__global__ __launch_bounds__(64) void pose_update(PoseArgs pa, PoseWs ws, int tiles, int it, int apply) {
#pragma clang fp contract(off)
    const int b = blockIdx.x, lane = threadIdx.x;
    double s[kPS];
    image_tile_sums(ws.part + (size_t)b * tiles * kPS, tiles, lane, s);
    const int* cb = ws.cnt + (size_t)b * tiles;
    int n = 0;
    for (int t = lane; t < tiles; t += 64) n += cb[t];
    n = wave_sum(n);
    if (lane != 0) return;
#pragma unroll
    for (int k = 0; k < kPS; ++k) ws.sums[(size_t)b * kPS + k] = s[k];
    const double den = (double)pa.w.C * (double)max(n, 1);
    pa.cost[(size_t)b * pa.history + it] = (float)(s[27] / den);
    pa.n[(size_t)b * pa.history + it] = n;
    if (!apply) return;

    // A = H + damping diag(H), symmetric, from the upper triangle. Every loop below has constant bounds and is
    // unrolled, so the arrays are registers (no scratch).
    double A[6][6], g[6];
    {
        int o = 0;
#pragma unroll
        for (int k = 0; k < 6; ++k) {
#pragma unroll
            for (int l = k; l < 6; ++l, ++o) A[k][l] = s[o], A[l][k] = s[o];
        }
        const double damping = (double)pa.damping;
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            const double dk = damping * A[k][k];
            A[k][k] = A[k][k] + dk;
            g[k] = -s[21 + k];
        }
    }
    // A = L D L^T, row by row; v[k] = L[j][k] D[k]. After a bad pivot the rest is computed and discarded.
    int status = n < pa.min_points ? 1 : 0;
    double L[6][6], D[6], delta[6];
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        double v[6];
        double d = A[j][j];
#pragma unroll
        for (int k = 0; k < j; ++k) {
            v[k] = L[j][k] * D[k];
            const double lv = L[j][k] * v[k];
            d = d - lv;
        }
        if (status == 0 && (!(d > 0.0) || !(d <= 1.7976931348623157e308))) status = 2;
        D[j] = d;
#pragma unroll
        for (int i = j + 1; i < 6; ++i) {
            double e = A[i][j];
#pragma unroll
            for (int k = 0; k < j; ++k) {
                const double lv = L[i][k] * v[k];
                e = e - lv;
            }
            L[i][j] = e / d;
        }
    }
    {
        double y[6];
#pragma unroll
        for (int i = 0; i < 6; ++i) {  // L y = g
            double e = g[i];
#pragma unroll
            for (int k = 0; k < i; ++k) {
                const double ly = L[i][k] * y[k];
                e = e - ly;
            }
            y[i] = e;
        }
#pragma unroll
        for (int i = 5; i >= 0; --i) {  // L^T delta = D^-1 y
            double e = y[i] / D[i];
#pragma unroll
            for (int k = i + 1; k < 6; ++k) {
                const double ld = L[k][i] * delta[k];
                e = e - ld;
            }
            delta[i] = e;
        }
#pragma unroll
        for (int k = 0; k < 6; ++k)
            if (status == 0 && !(fabs(delta[k]) <= 1.7976931348623157e308)) status = 3;
    }
    pa.status[b] = status;
    double* P = ws.state + (size_t)b * 12;
    double R[3][4];
#pragma unroll
    for (int k = 0; k < 12; ++k) R[k / 4][k % 4] = P[k];
    if (status == 0) {
        // the Cayley retraction of omega = delta[3..5]: dR = I + (2 / (1 + a.a)) ([a]x + [a]x^2), a = omega / 2
        const double a0 = delta[3] / 2.0, a1 = delta[4] / 2.0, a2 = delta[5] / 2.0;
        const double q00 = a0 * a0, q11 = a1 * a1, q22 = a2 * a2;
        const double q01 = a0 * a1, q02 = a0 * a2, q12 = a1 * a2;
        const double nn = (q00 + q11) + q22;
        const double f = 2.0 / (1.0 + nn);
        double dR[3][3];
        dR[0][0] = 1.0 + f * (-(q11 + q22));
        dR[0][1] = f * (-a2 + q01);
        dR[0][2] = f * (a1 + q02);
        dR[1][0] = f * (a2 + q01);
        dR[1][1] = 1.0 + f * (-(q00 + q22));
        dR[1][2] = f * (-a0 + q12);
        dR[2][0] = f * (-a1 + q02);
        dR[2][1] = f * (a0 + q12);
        dR[2][2] = 1.0 + f * (-(q00 + q11));
        double N[3][4];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const double p0 = dR[i][0] * R[0][j], p1 = dR[i][1] * R[1][j], p2 = dR[i][2] * R[2][j];
                const double s01 = p0 + p1;
                N[i][j] = s01 + p2;
            }
        }
#pragma unroll
        for (int i = 0; i < 3; ++i) N[i][3] = N[i][3] + delta[i];
#pragma unroll
        for (int k = 0; k < 12; ++k) R[k / 4][k % 4] = N[k / 4][k % 4], P[k] = N[k / 4][k % 4];
    }
    // the fp32 pose and m = K_src [R | t], each entry rounded once
    const float* ks = pa.k_src + (long long)b * pa.ksbs;
    float* po = pa.pose + (size_t)b * 12;
    float* mo = pa.m_out + (long long)b * pa.w.mbs;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            po[i * 4 + j] = (float)R[i][j];
            const double p0 = (double)ks[i * 3 + 0] * R[0][j], p1 = (double)ks[i * 3 + 1] * R[1][j],
                         p2 = (double)ks[i * 3 + 2] * R[2][j];
            const double s01 = p0 + p1;
            mo[i * 4 + j] = (float)(s01 + p2);
        }
    }
}

}  // namespace

size_t pose_workspace_bytes(int B, int H, int W) {
    // pose_ws: state, sums (doubles), part, cnt
    return (size_t)B * (12 + kPS) * 8 + (size_t)B * loss_tiles_per_image(H, W) * (kPS + 1) * 4;
}

int launch_pose_normal_eq(const PoseArgs& a, void* ws, hipStream_t st, const char** why) {
    const int tiles = loss_tiles_per_image(a.w.H, a.w.W);
    const PoseWs p = pose_ws(ws, a.w.B, tiles);
    const dim3 g(a.w.B * tiles), t(kWT);
    if (a.w.C == 1)
        hipLaunchKernelGGL(pose_normal_eq<1>, g, t, 0, st, a, p.part, p.cnt);
    else
        hipLaunchKernelGGL(pose_normal_eq<3>, g, t, 0, st, a, p.part, p.cnt);
    return launch_status(why);
}

int launch_pose_update(const PoseArgs& a, void* ws, int it, int apply, hipStream_t st, const char** why) {
    const int tiles = loss_tiles_per_image(a.w.H, a.w.W);
    const PoseWs p = pose_ws(ws, a.w.B, tiles);
    hipLaunchKernelGGL(pose_update, dim3(a.w.B), dim3(64), 0, st, a, p, tiles, it, apply);
    return launch_status(why);
}

}  // namespace nconv
