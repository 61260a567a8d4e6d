// Body-model path of a ProHMR-style multi-hypothesis head (reference README.md:26-42):
//   6D rotation representation -> R   (hand/manopth/rot6d.py:4-24 Gram-Schmidt form, :26-51 symmetric 'robust' form; used by
//                                      hand/manopth/manolayer.py:150-156) and its reverse,
//   linear-blend skinning for a model of runtime size (J <= 32 joints, V vertices, nb shape / 9(J-1) pose-blend coefficients,
//   any kinematic tree with parents[j] < j): the arithmetic of hand/manopth/manolayer.py:181-246 at other sizes
//   (SMPL: 24 joints, 6,890 vertices, 207 pose-blend coefficients).
// Two launches like the hand mesh (mano.hip): a pose kernel (one wavefront per hypothesis: rest joints, kinematic chain, skinning
// transforms, pose map -> one workspace row) and a skinning kernel (one thread per vertex, HB hypotheses per workgroup, every
// per-hypothesis value a wave-uniform scalar operand, blend-shape tables read vertex-fastest and reused across the HB hypotheses).
// Algorithmic bytes per hypothesis: 12 V written (+ workspace row); 3 V (nb + 9(J-1) + 4 J + 4) FMA.
#include "common.h"

namespace mhe { namespace body {

__device__ __forceinline__ void cross3(const float *u, const float *v, float *o) {
    o[0] = u[1] * v[2] - u[2] * v[1]; o[1] = u[2] * v[0] - u[0] * v[2]; o[2] = u[0] * v[1] - u[1] * v[0];
}
__device__ __forceinline__ float norm3c(const float *v) { return fmaxf(sqrtf(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]), 1e-8f); }   // rot6d.py:54-60

__global__ void rot6d_kernel(const float *__restrict__ p6, float *__restrict__ Rm, long n, int robust) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float a[3], b[3], x[3], y[3], z[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) { a[c] = p6[i * 6 + c]; b[c] = p6[i * 6 + 3 + c]; }
    if (!robust) {                       // x = n(a), z = n(x x b), y = z x x
        const float na = norm3c(a);
#pragma unroll
        for (int c = 0; c < 3; ++c) x[c] = a[c] / na;
        float t[3];
        cross3(x, b, t);
        const float nt = norm3c(t);
#pragma unroll
        for (int c = 0; c < 3; ++c) z[c] = t[c] / nt;
        cross3(z, x, y);
    } else {                             // symmetric: orthogonalise the normalised pair around its bisector
        const float na = norm3c(a), nb = norm3c(b);
        float m[3], o[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) { x[c] = a[c] / na; y[c] = b[c] / nb; m[c] = x[c] + y[c]; o[c] = x[c] - y[c]; }
        const float nm = norm3c(m), no = norm3c(o);
#pragma unroll
        for (int c = 0; c < 3; ++c) { m[c] /= nm; o[c] /= no; x[c] = m[c] + o[c]; y[c] = m[c] - o[c]; }
        const float nx = norm3c(x), ny = norm3c(y);
#pragma unroll
        for (int c = 0; c < 3; ++c) { x[c] /= nx; y[c] /= ny; }
        float t[3];
        cross3(x, y, t);
        const float nt = norm3c(t);
#pragma unroll
        for (int c = 0; c < 3; ++c) z[c] = t[c] / nt;
    }
#pragma unroll
    for (int r = 0; r < 3; ++r) { Rm[i * 9 + 3 * r] = x[r]; Rm[i * 9 + 3 * r + 1] = y[r]; Rm[i * 9 + 3 * r + 2] = z[r]; }   // columns x, y, z
}

// reverse of the Gram-Schmidt form: g6 = (dR/dp6)^T gR
__global__ void rot6d_bwd_kernel(const float *__restrict__ p6, const float *__restrict__ gR, float *__restrict__ g6, long n) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float a[3], b[3], x[3], z[3], t[3], gx[3], gy[3], gz[3], tmp[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        a[c] = p6[i * 6 + c]; b[c] = p6[i * 6 + 3 + c];
        gx[c] = gR[i * 9 + 3 * c]; gy[c] = gR[i * 9 + 3 * c + 1]; gz[c] = gR[i * 9 + 3 * c + 2];
    }
    const float ra = sqrtf(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]), na = fmaxf(ra, 1e-8f);
#pragma unroll
    for (int c = 0; c < 3; ++c) x[c] = a[c] / na;
    cross3(x, b, t);
    const float rt = sqrtf(t[0] * t[0] + t[1] * t[1] + t[2] * t[2]), nt = fmaxf(rt, 1e-8f);
#pragma unroll
    for (int c = 0; c < 3; ++c) z[c] = t[c] / nt;
    // y = z x x :  gz += x x gy,  gx += gy x z
    cross3(x, gy, tmp);
#pragma unroll
    for (int c = 0; c < 3; ++c) gz[c] += tmp[c];
    cross3(gy, z, tmp);
#pragma unroll
    for (int c = 0; c < 3; ++c) gx[c] += tmp[c];
    // z = t / max(|t|, eps)
    float gt[3];
    const float dz = rt > 1e-8f ? z[0] * gz[0] + z[1] * gz[1] + z[2] * gz[2] : 0.f;
#pragma unroll
    for (int c = 0; c < 3; ++c) gt[c] = (gz[c] - z[c] * dz) / nt;
    // t = x x b :  gx += b x gt,  gb = gt x x
    float gb[3];
    cross3(b, gt, tmp);
#pragma unroll
    for (int c = 0; c < 3; ++c) gx[c] += tmp[c];
    cross3(gt, x, gb);
    const float dx = ra > 1e-8f ? x[0] * gx[0] + x[1] * gx[1] + x[2] * gx[2] : 0.f;
#pragma unroll
    for (int c = 0; c < 3; ++c) { g6[i * 6 + c] = (gx[c] - x[c] * dx) / na; g6[i * 6 + 3 + c] = gb[c]; }
}

// workspace row: pose map [9(J-1)] | betas [nb] | skinning transforms [J][12] (3x3 row-major, then translation) | posed joints [J][3]
__host__ __device__ inline int ws_pm(int, int) { return 0; }
__host__ __device__ inline int ws_bt(int J, int) { return 9 * (J - 1); }
__host__ __device__ inline int ws_a(int J, int nb) { return 9 * (J - 1) + nb; }
__host__ __device__ inline int ws_jp(int J, int nb) { return 9 * (J - 1) + nb + 12 * J; }
__host__ __device__ inline int ws_stride(int J, int nb) { return (9 * (J - 1) + nb + 15 * J + 15) / 16 * 16; }
constexpr int MAXJ = 32;

__global__ __launch_bounds__(256) void lbs_pose_kernel(const float *__restrict__ rot, const float *__restrict__ betas,
                                                       const float *__restrict__ jt, const float *__restrict__ jsd,
                                                       const int *__restrict__ parents, float *__restrict__ ws,
                                                       float *__restrict__ joints_o, int R, int J, int nb) {
    __shared__ float sG[4][MAXJ * 12], sJ[4][MAXJ * 3];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    float *G = sG[wave], *Jr = sJ[wave];
    const int stride = ws_stride(J, nb);
    for (int r = blockIdx.x * 4 + wave; r < R; r += gridDim.x * 4) {
        const float *Rr = rot + (size_t)r * J * 9, *bt = betas + (size_t)r * nb;
        float *w = ws + (size_t)r * stride;
        // rest joints: J_template + J_shapedirs beta  (manolayer.py:181-184, joint regression folded into the tables)
        for (int e = lane; e < 3 * J; e += 64) {
            float v = jt[e];
            for (int k = 0; k < nb; ++k) v = fmaf(jsd[e * nb + k], bt[k], v);
            Jr[e] = v;
        }
        for (int e = lane; e < 9 * (J - 1); e += 64) {
            const int d = e % 9;
            w[ws_pm(J, nb) + e] = Rr[9 + e] - ((d == 0 || d == 4 || d == 8) ? 1.f : 0.f);                 // manolayer.py:187
        }
        if (lane < nb) w[ws_bt(J, nb) + lane] = bt[lane];
        wave_sync();
        // kinematic chain (manolayer.py:193-229): G_j = G_parent [R_j | j_j - j_parent]; lane e < 12 owns element (row e/4... ) of G_j
        if (lane < 12) {
            const int rr = lane / 4, cc = lane % 4;
            G[lane] = cc < 3 ? Rr[3 * rr + cc] : Jr[rr];
        }
        wave_sync();
        for (int j = 1; j < J; ++j) {
            const int p = parents[j];
            float v = 0.f;
            if (lane < 12) {
                const int rr = lane / 4, cc = lane % 4;
                const float *Gp = G + 12 * p;
                if (cc < 3) {
                    v = Gp[4 * rr] * Rr[9 * j + cc] + Gp[4 * rr + 1] * Rr[9 * j + 3 + cc] + Gp[4 * rr + 2] * Rr[9 * j + 6 + cc];
                } else {
                    const float t0 = Jr[3 * j] - Jr[3 * p], t1 = Jr[3 * j + 1] - Jr[3 * p + 1], t2 = Jr[3 * j + 2] - Jr[3 * p + 2];
                    v = Gp[4 * rr] * t0 + Gp[4 * rr + 1] * t1 + Gp[4 * rr + 2] * t2 + Gp[4 * rr + 3];
                }
            }
            wave_sync();
            if (lane < 12) G[12 * j + lane] = v;
            wave_sync();
        }
        // skinning transforms: rotation of G_j, translation G_j.t - G_j.R j_rest  (manolayer.py:231-234); posed joints = G_j.t
        for (int e = lane; e < 12 * J; e += 64) {
            const int j = e / 12, k = e % 12;
            const float *Gj = G + 12 * j;
            float v;
            if (k < 9) v = Gj[4 * (k / 3) + k % 3];
            else {
                const int rr = k - 9;
                v = Gj[4 * rr + 3] - (Gj[4 * rr] * Jr[3 * j] + Gj[4 * rr + 1] * Jr[3 * j + 1] + Gj[4 * rr + 2] * Jr[3 * j + 2]);
            }
            w[ws_a(J, nb) + e] = v;
        }
        for (int e = lane; e < 3 * J; e += 64) {
            const float v = G[12 * (e / 3) + 4 * (e % 3) + 3];
            w[ws_jp(J, nb) + e] = v;
            if (joints_o) joints_o[(size_t)r * 3 * J + e] = v;
        }
        wave_sync();
    }
}

// Reverse of the posed joints of lbs_pose_kernel (one wavefront per hypothesis): with Rw_j the world rotation and t_j = posed joint j,
//   Rw_j = Rw_p R_j,  t_j = Rw_p (J_j - J_p) + t_p  (p = parents[j]);  Rw_0 = R_0, t_0 = J_0;  J = j_template + j_shapedirs beta.
// The forward chain is recomputed into LDS, then walked child -> parent (j = J-1 .. 1, parents[j] < j: every child is done before its parent):
//   g_R_j = Rw_p^T gRw_j;  gRw_p += gRw_j R_j^T + gt_j (J_j - J_p)^T;  gt_p += gt_j;  gJ_j += Rw_p^T gt_j;  gJ_p -= Rw_p^T gt_j
// and g_beta = j_shapedirs^T gJ.  Lanes 0..8 own the 3x3 terms, lanes 9..11 the vectors: no two lanes write one LDS word within a step.
__global__ __launch_bounds__(256) void lbs_pose_bwd_kernel(const float *__restrict__ rot, const float *__restrict__ betas,
                                                           const float *__restrict__ jt, const float *__restrict__ jsd,
                                                           const int *__restrict__ parents, const float *__restrict__ g_joints,
                                                           float *__restrict__ g_rot, float *__restrict__ g_betas, int R, int J, int nb) {
    __shared__ float sW[4][MAXJ * 9], sJ[4][MAXJ * 3], sGW[4][MAXJ * 9], sGT[4][MAXJ * 3], sGJ[4][MAXJ * 3];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    float *W = sW[wave], *Jr = sJ[wave], *GW = sGW[wave], *GT = sGT[wave], *GJ = sGJ[wave];
    for (int r = blockIdx.x * 4 + wave; r < R; r += gridDim.x * 4) {
        const float *Rr = rot + (size_t)r * J * 9, *bt = betas + (size_t)r * nb;
        for (int e = lane; e < 3 * J; e += 64) {
            float v = jt[e];
            for (int k = 0; k < nb; ++k) v = fmaf(jsd[e * nb + k], bt[k], v);
            Jr[e] = v;
            GT[e] = g_joints[(size_t)r * 3 * J + e];
            GJ[e] = 0.f;
        }
        for (int e = lane; e < 9 * J; e += 64) GW[e] = 0.f;
        if (lane < 9) W[lane] = Rr[lane];
        wave_sync();
        for (int j = 1; j < J; ++j) {                     // world rotations
            const int p = parents[j];
            if (lane < 9) {
                const int a = lane / 3, b = lane % 3;
                W[9 * j + lane] = W[9 * p + 3 * a] * Rr[9 * j + b] + W[9 * p + 3 * a + 1] * Rr[9 * j + 3 + b] + W[9 * p + 3 * a + 2] * Rr[9 * j + 6 + b];
            }
            wave_sync();
        }
        for (int j = J - 1; j >= 1; --j) {
            const int p = parents[j];
            const float *Wp = W + 9 * p, *gw = GW + 9 * j, *gt = GT + 3 * j, *Rj = Rr + 9 * j;
            if (lane < 9) {
                const int a = lane / 3, b = lane % 3;
                g_rot[(size_t)r * J * 9 + 9 * j + lane] = Wp[a] * gw[b] + Wp[3 + a] * gw[3 + b] + Wp[6 + a] * gw[6 + b];
                GW[9 * p + lane] += gw[3 * a] * Rj[3 * b] + gw[3 * a + 1] * Rj[3 * b + 1] + gw[3 * a + 2] * Rj[3 * b + 2] + gt[a] * (Jr[3 * j + b] - Jr[3 * p + b]);
            } else if (lane < 12) {
                const int c = lane - 9;
                const float u = Wp[c] * gt[0] + Wp[3 + c] * gt[1] + Wp[6 + c] * gt[2];
                GJ[3 * j + c] += u;
                GJ[3 * p + c] -= u;
                GT[3 * p + c] += gt[c];
            }
            wave_sync();
        }
        if (lane < 9) g_rot[(size_t)r * J * 9 + lane] = GW[lane];
        else if (lane < 12) GJ[lane - 9] += GT[lane - 9];
        wave_sync();
        if (lane < nb) {
            float a = 0.f;
            for (int e = 0; e < 3 * J; ++e) a = fmaf(jsd[e * nb + lane], GJ[e], a);
            g_betas[(size_t)r * nb + lane] = a;
        }
        wave_sync();
    }
}

// Reverse of the whole pose pass (one wavefront per hypothesis): the gradients of the skinning transforms A_j = [Rw_j | a_j], a_j = t_j - Rw_j J_j
// (g_transforms [J][12], the workspace layout), of the pose map p = R_j - I (g_posemap [9(J-1)]) and optionally of the posed joints seed
//   gRw_j = gA_j[:, :3] - g_a_j J_j^T,  gt_j = g_joints_j + g_a_j,  gJ_j = -Rw_j^T g_a_j
// then the child -> parent walk of lbs_pose_bwd_kernel, with g_R_j += g_posemap[block j - 1]; g_beta = g_betas_in + j_shapedirs^T gJ.
// g_betas_in may be g_betas (each lane reads its element before writing it).
__global__ __launch_bounds__(256) void lbs_transforms_bwd_kernel(const float *__restrict__ rot, const float *__restrict__ betas,
                                                                 const float *__restrict__ jt, const float *__restrict__ jsd,
                                                                 const int *__restrict__ parents, const float *__restrict__ g_joints,
                                                                 const float *__restrict__ g_tf, const float *__restrict__ g_pm, const float *g_betas_in,
                                                                 float *__restrict__ g_rot, float *g_betas, int R, int J, int nb) {
    __shared__ float sW[4][MAXJ * 9], sJ[4][MAXJ * 3], sGW[4][MAXJ * 9], sGT[4][MAXJ * 3], sGJ[4][MAXJ * 3];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    float *W = sW[wave], *Jr = sJ[wave], *GW = sGW[wave], *GT = sGT[wave], *GJ = sGJ[wave];
    for (int r = blockIdx.x * 4 + wave; r < R; r += gridDim.x * 4) {
        const float *Rr = rot + (size_t)r * J * 9, *bt = betas + (size_t)r * nb, *ga = g_tf + (size_t)r * J * 12, *gp = g_pm + (size_t)r * 9 * (J - 1);
        for (int e = lane; e < 3 * J; e += 64) {
            float v = jt[e];
            for (int k = 0; k < nb; ++k) v = fmaf(jsd[e * nb + k], bt[k], v);
            Jr[e] = v;
        }
        if (lane < 9) W[lane] = Rr[lane];
        wave_sync();
        for (int j = 1; j < J; ++j) {                     // world rotations
            const int p = parents[j];
            if (lane < 9) {
                const int a = lane / 3, b = lane % 3;
                W[9 * j + lane] = W[9 * p + 3 * a] * Rr[9 * j + b] + W[9 * p + 3 * a + 1] * Rr[9 * j + 3 + b] + W[9 * p + 3 * a + 2] * Rr[9 * j + 6 + b];
            }
            wave_sync();
        }
        for (int e = lane; e < 9 * J; e += 64) {
            const int j = e / 9, k = e % 9;
            GW[e] = ga[j * 12 + k] - ga[j * 12 + 9 + k / 3] * Jr[3 * j + k % 3];
        }
        for (int e = lane; e < 3 * J; e += 64) {
            const int j = e / 3, c = e % 3;
            const float *g = ga + j * 12 + 9, *Wj = W + 9 * j;
            GT[e] = (g_joints ? g_joints[(size_t)r * 3 * J + e] : 0.f) + g[c];
            GJ[e] = -(Wj[c] * g[0] + Wj[3 + c] * g[1] + Wj[6 + c] * g[2]);
        }
        wave_sync();
        for (int j = J - 1; j >= 1; --j) {
            const int p = parents[j];
            const float *Wp = W + 9 * p, *gw = GW + 9 * j, *gt = GT + 3 * j, *Rj = Rr + 9 * j;
            if (lane < 9) {
                const int a = lane / 3, b = lane % 3;
                g_rot[(size_t)r * J * 9 + 9 * j + lane] = Wp[a] * gw[b] + Wp[3 + a] * gw[3 + b] + Wp[6 + a] * gw[6 + b] + gp[9 * (j - 1) + lane];
                GW[9 * p + lane] += gw[3 * a] * Rj[3 * b] + gw[3 * a + 1] * Rj[3 * b + 1] + gw[3 * a + 2] * Rj[3 * b + 2] + gt[a] * (Jr[3 * j + b] - Jr[3 * p + b]);
            } else if (lane < 12) {
                const int c = lane - 9;
                const float u = Wp[c] * gt[0] + Wp[3 + c] * gt[1] + Wp[6 + c] * gt[2];
                GJ[3 * j + c] += u;
                GJ[3 * p + c] -= u;
                GT[3 * p + c] += gt[c];
            }
            wave_sync();
        }
        if (lane < 9) g_rot[(size_t)r * J * 9 + lane] = GW[lane];
        else if (lane < 12) GJ[lane - 9] += GT[lane - 9];
        wave_sync();
        if (lane < nb) {
            float a = g_betas_in ? g_betas_in[(size_t)r * nb + lane] : 0.f;
            for (int e = 0; e < 3 * J; ++e) a = fmaf(jsd[e * nb + lane], GJ[e], a);
            g_betas[(size_t)r * nb + lane] = a;
        }
        wave_sync();
    }
}

// vertex vc (< NV) of hypotheses r0 .. r0 + HB - 1 (rows past R: row R - 1 again): out[h][c], scaled
template <int HB>
__device__ __forceinline__ void lbs_skin_vertex(const float *__restrict__ ws, const float *__restrict__ Vt, const float *__restrict__ Vsd,
                                                const float *__restrict__ Vpd, const float *__restrict__ Vw, int r0, int vc, int R, int J, int nb, int VP,
                                                float scale, float (&out)[HB][3]) {
    const int stride = ws_stride(J, nb), NP = 9 * (J - 1), oa = ws_a(J, nb), ob = ws_bt(J, nb);
    const float *wrow[HB];
#pragma unroll
    for (int h = 0; h < HB; ++h) wrow[h] = ws + (size_t)(r0 + h < R ? r0 + h : R - 1) * stride;
    float acc[HB][3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float t = Vt[c * VP + vc];
#pragma unroll
        for (int h = 0; h < HB; ++h) acc[h][c] = t;
    }
    for (int k = 0; k < nb; ++k) {                 // shape blend (manolayer.py:181-183)
        const float s0 = Vsd[(k * 3 + 0) * VP + vc], s1 = Vsd[(k * 3 + 1) * VP + vc], s2 = Vsd[(k * 3 + 2) * VP + vc];
#pragma unroll
        for (int h = 0; h < HB; ++h) {
            const float bk = wrow[h][ob + k];
            acc[h][0] = fmaf(s0, bk, acc[h][0]); acc[h][1] = fmaf(s1, bk, acc[h][1]); acc[h][2] = fmaf(s2, bk, acc[h][2]);
        }
    }
#pragma unroll 3
    for (int k = 0; k < NP; ++k) {                 // pose-corrective blend (:187-188)
        const float p0 = Vpd[(k * 3 + 0) * VP + vc], p1 = Vpd[(k * 3 + 1) * VP + vc], p2 = Vpd[(k * 3 + 2) * VP + vc];
#pragma unroll
        for (int h = 0; h < HB; ++h) {
            const float m = wrow[h][k];
            acc[h][0] = fmaf(p0, m, acc[h][0]); acc[h][1] = fmaf(p1, m, acc[h][1]); acc[h][2] = fmaf(p2, m, acc[h][2]);
        }
    }
    float T[HB][12];
#pragma unroll
    for (int h = 0; h < HB; ++h)
#pragma unroll
        for (int e = 0; e < 12; ++e) T[h][e] = 0.f;
    for (int j = 0; j < J; ++j) {                  // T = sum_j w_j A_j  (:236)
        const float wj = Vw[j * VP + vc];
#pragma unroll
        for (int h = 0; h < HB; ++h)
#pragma unroll
            for (int e = 0; e < 12; ++e) T[h][e] = fmaf(wrow[h][oa + j * 12 + e], wj, T[h][e]);
    }
#pragma unroll
    for (int h = 0; h < HB; ++h)
#pragma unroll
        for (int c = 0; c < 3; ++c)
            out[h][c] = affine_row(T[h][3 * c], acc[h][0], T[h][3 * c + 1], acc[h][1], T[h][3 * c + 2], acc[h][2], T[h][9 + c], scale);   // :245-246
}

template <int HB>
__global__ __launch_bounds__(256) void lbs_skin_kernel(const float *__restrict__ ws, const float *__restrict__ Vt, const float *__restrict__ Vsd,
                                                       const float *__restrict__ Vpd, const float *__restrict__ Vw, float *__restrict__ verts_o,
                                                       int R, int J, int nb, int NV, int VP, float scale) {
    const int v = blockIdx.x * 256 + threadIdx.x;
    const int r0 = blockIdx.y * HB;
    float out[HB][3];
    lbs_skin_vertex<HB>(ws, Vt, Vsd, Vpd, Vw, r0, v < NV ? v : NV - 1, R, J, nb, VP, scale, out);
#pragma unroll
    for (int h = 0; h < HB; ++h) {
        const int r = r0 + h;
        if (v < NV && r < R) {
#pragma unroll
            for (int c = 0; c < 3; ++c) verts_o[((size_t)r * NV + v) * 3 + c] = out[h][c];
        }
    }
}

// The same skinning with the keypoints (regressor (NK, NV) x scaled vertices) accumulated inside the pass: one workgroup walks ALL vertex blocks
// for its HB hypotheses; per block of 256 vertices the vertices and the regressor's columns go through LDS and thread t adds the block's 256
// terms, in order, to its (hypothesis, coordinate, keypoint) sums t, t + 256, ... (at most HB * 64 * 3 / 256 = 6), which stay in registers
// across the vertex loop and are stored once: fixed summation order, no atomics.  verts_o may be null (no vertex tensor is written).
// Dynamic LDS: (HB * 3 * 256 + NK * 257) floats.
template <int HB>
__global__ __launch_bounds__(256) void lbs_skin_kp_kernel(const float *__restrict__ ws, const float *__restrict__ Vt, const float *__restrict__ Vsd,
                                                          const float *__restrict__ Vpd, const float *__restrict__ Vw, const float *__restrict__ reg,
                                                          float *__restrict__ verts_o, float *__restrict__ kp_o, int R, int J, int nb, int NV, int VP,
                                                          int NK, float scale) {
    extern __shared__ float kp_smem[];
    float *sV = kp_smem, *sR = kp_smem + HB * 3 * 256;          // [HB * 3][256], [NK][257]
    constexpr int NQ = HB * 64 * 3 / 256;
    const int tid = threadIdx.x, r0 = blockIdx.x * HB, NC = HB * 3 * NK;
    float sum[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) sum[q] = 0.f;
    for (int v0 = 0; v0 < NV; v0 += 256) {
        const int v = v0 + tid;
        float out[HB][3];
        lbs_skin_vertex<HB>(ws, Vt, Vsd, Vpd, Vw, r0, v < NV ? v : NV - 1, R, J, nb, VP, scale, out);
        __syncthreads();                                        // the previous block's sums are done with sV / sR
#pragma unroll
        for (int h = 0; h < HB; ++h) {
#pragma unroll
            for (int c = 0; c < 3; ++c) sV[(h * 3 + c) * 256 + tid] = v < NV ? out[h][c] : 0.f;
            if (verts_o && v < NV && r0 + h < R) {
#pragma unroll
                for (int c = 0; c < 3; ++c) verts_o[((size_t)(r0 + h) * NV + v) * 3 + c] = out[h][c];
            }
        }
        for (int k = 0; k < NK; ++k) sR[k * 257 + tid] = v < NV ? reg[(size_t)k * NV + v] : 0.f;
        __syncthreads();
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const int idx = tid + 256 * q;
            if (idx < NC) {
                const float *a = sV + (idx / NK) * 256, *b = sR + (idx % NK) * 257;
                float t = sum[q];
                for (int i = 0; i < 256; ++i) t = fmaf(b[i], a[i], t);
                sum[q] = t;
            }
        }
    }
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        const int idx = tid + 256 * q;
        if (idx < NC) {
            const int hc = idx / NK, k = idx - hc * NK, h = hc / 3, c = hc - 3 * h;
            if (r0 + h < R) kp_o[((size_t)(r0 + h) * NK + k) * 3 + c] = sum[q];
        }
    }
}

// The same skinning with the mesh error accumulated inside the pass (no vertex tensor): err[r] = mean_v || scale vert[r][v] - center[r] -
// target[r / rpi][v] ||.  One workgroup walks all vertex blocks for its HB hypotheses; thread t keeps HB sums over the vertices t, t + 256, ...
// (a thread past NV adds exactly 0 and re-reads vertex NV - 1 of the target, never beyond it); then per hypothesis 16 threads add 16 consecutive
// threads' sums each, in order, and one thread adds those 16, in order: fixed summation order, no atomics.  One division by NV at the end.
template <int HB>
__global__ __launch_bounds__(256) void lbs_skin_err_kernel(const float *__restrict__ ws, const float *__restrict__ Vt, const float *__restrict__ Vsd,
                                                           const float *__restrict__ Vpd, const float *__restrict__ Vw, const float *__restrict__ tgt,
                                                           const float *__restrict__ center, float *__restrict__ err_o, int R, int J, int nb, int NV,
                                                           int VP, int rpi, float scale) {
    __shared__ float sE[HB][256], sP[HB][16], sC[HB][3];
    __shared__ size_t sT[HB];                                   // the hypotheses' centres and target offsets (registers go to the skinning)
    const int tid = threadIdx.x, r0 = blockIdx.x * HB;
    if (tid < HB * 3) {
        const int h = tid / 3, r = r0 + h < R ? r0 + h : R - 1;
        sC[h][tid - 3 * h] = center ? center[(size_t)r * 3 + (tid - 3 * h)] : 0.f;
        if (tid == 3 * h) sT[h] = (size_t)(r / rpi) * NV * 3;
    }
    __syncthreads();
    float sum[HB];
#pragma unroll
    for (int h = 0; h < HB; ++h) sum[h] = 0.f;
    for (int v0 = 0; v0 < NV; v0 += 256) {
        const int v = v0 + tid, vc = v < NV ? v : NV - 1;
        float out[HB][3];
        lbs_skin_vertex<HB>(ws, Vt, Vsd, Vpd, Vw, r0, vc, R, J, nb, VP, scale, out);
#pragma unroll
        for (int h = 0; h < HB; ++h) {
            float sq = 0.f;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float d = (out[h][c] - sC[h][c]) - tgt[sT[h] + vc * 3 + c];
                sq = c == 0 ? d * d : fmaf(d, d, sq);
            }
            sum[h] += v < NV ? sqrtf(sq) : 0.f;
        }
    }
#pragma unroll
    for (int h = 0; h < HB; ++h) sE[h][tid] = sum[h];
    __syncthreads();
    if (tid < HB * 16) {
        const float *q = &sE[tid >> 4][(tid & 15) * 16];
        float a = q[0];
        for (int i = 1; i < 16; ++i) a += q[i];
        sP[tid >> 4][tid & 15] = a;
    }
    __syncthreads();
    if (tid < HB && r0 + tid < R) {
        float a = sP[tid][0];
        for (int i = 1; i < 16; ++i) a += sP[tid][i];
        err_o[r0 + tid] = a / (float)NV;
    }
}

}}  // namespace mhe::body

using namespace mhe;

extern "C" int mhe_rot6d_to_rotmat_f32(const float *poses6, float *rotmats, long n, int robust, void *stream) {
    MHE_REQUIRE(poses6 && rotmats && n > 0, "mhe_rot6d_to_rotmat_f32: bad arguments");
    hipLaunchKernelGGL(body::rot6d_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, poses6, rotmats, n, robust);
    return check_launch("rot6d_kernel");
}

extern "C" int mhe_rot6d_to_rotmat_bwd_f32(const float *poses6, const float *g_rotmats, float *g_poses6, long n, void *stream) {
    MHE_REQUIRE(poses6 && g_rotmats && g_poses6 && n > 0, "mhe_rot6d_to_rotmat_bwd_f32: bad arguments");
    hipLaunchKernelGGL(body::rot6d_bwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, poses6, g_rotmats, g_poses6, n);
    return check_launch("rot6d_bwd_kernel");
}

extern "C" size_t mhe_lbs_workspace_floats(int R, int J, int nb) {
    return (R > 0 && J > 0 && J <= body::MAXJ && nb >= 0) ? (size_t)R * body::ws_stride(J, nb) : 0;
}

extern "C" int mhe_lbs_pose_f32(const float *rotmats, const float *betas, const float *j_template, const float *j_shapedirs,
                                const int *parents, float *workspace, float *joints, int R, int J, int nb, void *stream) {
    MHE_REQUIRE(rotmats && betas && j_template && j_shapedirs && parents && workspace, "mhe_lbs_pose_f32: null pointer");
    MHE_REQUIRE(R > 0 && J > 0 && J <= body::MAXJ && nb > 0 && nb <= 64, "mhe_lbs_pose_f32: R=%d J=%d nb=%d", R, J, nb);
    const int blocks = (R + 3) / 4 < 2048 ? (R + 3) / 4 : 2048;
    hipLaunchKernelGGL(body::lbs_pose_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, rotmats, betas, j_template, j_shapedirs, parents,
                       workspace, joints, R, J, nb);
    return check_launch("lbs_pose_kernel");
}

extern "C" int mhe_lbs_pose_bwd_f32(const float *rotmats, const float *betas, const float *j_template, const float *j_shapedirs, const int *parents,
                                    const float *g_joints, float *g_rotmats, float *g_betas, int R, int J, int nb, void *stream) {
    MHE_REQUIRE(R > 0 && J > 0 && J <= body::MAXJ && nb > 0 && nb <= 64, "mhe_lbs_pose_bwd_f32: R=%d J=%d nb=%d", R, J, nb);
    MHE_REQUIRE(on_device(rotmats) && on_device(betas) && on_device(j_template) && on_device(j_shapedirs) && on_device(parents) && on_device(g_joints) &&
                    on_device(g_rotmats) && on_device(g_betas), "mhe_lbs_pose_bwd_f32: every buffer must be device memory");
    const int blocks = (R + 3) / 4 < 2048 ? (R + 3) / 4 : 2048;
    hipLaunchKernelGGL(body::lbs_pose_bwd_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, rotmats, betas, j_template, j_shapedirs, parents,
                       g_joints, g_rotmats, g_betas, R, J, nb);
    return check_launch("lbs_pose_bwd_kernel");
}

extern "C" int mhe_lbs_transforms_bwd_f32(const float *rotmats, const float *betas, const float *j_template, const float *j_shapedirs,
                                          const int *parents, const float *g_joints, const float *g_transforms, const float *g_posemap,
                                          const float *g_betas_in, float *g_rotmats, float *g_betas, int R, int J, int nb, void *stream) {
    MHE_REQUIRE(rotmats && betas && j_template && j_shapedirs && parents && g_transforms && g_posemap && g_rotmats && g_betas,
                "mhe_lbs_transforms_bwd_f32: null pointer");
    MHE_REQUIRE(R > 0 && J > 1 && J <= body::MAXJ && nb > 0 && nb <= 64, "mhe_lbs_transforms_bwd_f32: R=%d J=%d nb=%d", R, J, nb);
    MHE_REQUIRE(on_device(rotmats) && on_device(betas) && on_device(j_template) && on_device(j_shapedirs) && on_device(parents) &&
                    (!g_joints || on_device(g_joints)) && on_device(g_transforms) && on_device(g_posemap) && (!g_betas_in || on_device(g_betas_in)) &&
                    on_device(g_rotmats) && on_device(g_betas), "mhe_lbs_transforms_bwd_f32: every buffer must be device memory");
    const int blocks = (R + 3) / 4 < 2048 ? (R + 3) / 4 : 2048;
    hipLaunchKernelGGL(body::lbs_transforms_bwd_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, rotmats, betas, j_template, j_shapedirs,
                       parents, g_joints, g_transforms, g_posemap, g_betas_in, g_rotmats, g_betas, R, J, nb);
    return check_launch("lbs_transforms_bwd_kernel");
}

extern "C" int mhe_lbs_skin_f32(const float *workspace, const float *v_template, const float *v_shapedirs, const float *v_posedirs,
                                const float *v_weights, float *verts, int R, int J, int nb, int NV, int VP, float scale, void *stream) {
    MHE_REQUIRE(workspace && v_template && v_shapedirs && v_posedirs && v_weights && verts, "mhe_lbs_skin_f32: null pointer");
    MHE_REQUIRE(R > 0 && J > 0 && J <= body::MAXJ && nb > 0 && NV > 0 && VP >= NV, "mhe_lbs_skin_f32: R=%d J=%d nb=%d NV=%d VP=%d", R, J, nb, NV, VP);
    constexpr int HB = 8;
    hipLaunchKernelGGL(body::lbs_skin_kernel<HB>, dim3((NV + 255) / 256, (R + HB - 1) / HB), dim3(256), 0, (hipStream_t)stream, workspace,
                       v_template, v_shapedirs, v_posedirs, v_weights, verts, R, J, nb, NV, VP, scale);
    return check_launch("lbs_skin_kernel");
}

extern "C" int mhe_lbs_skin_kp_f32(const float *workspace, const float *v_template, const float *v_shapedirs, const float *v_posedirs,
                                   const float *v_weights, const float *regressor, float *verts, float *keypoints, int R, int J, int nb, int NV, int VP,
                                   int NK, float scale, void *stream) {
    MHE_REQUIRE(NK >= 1 && NK <= 64, "mhe_lbs_skin_kp_f32: NK=%d outside 1..64", NK);
    MHE_REQUIRE(workspace && v_template && v_shapedirs && v_posedirs && v_weights && regressor && keypoints,
                "mhe_lbs_skin_kp_f32: null pointer (only verts may be null)");
    MHE_REQUIRE(R > 0 && J > 0 && J <= body::MAXJ && nb > 0 && NV > 0 && VP >= NV, "mhe_lbs_skin_kp_f32: R=%d J=%d nb=%d NV=%d VP=%d", R, J, nb, NV, VP);
    constexpr int HB = 8;
    const int lds = (HB * 3 * 256 + NK * 257) * (int)sizeof(float);
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(body::lbs_skin_kp_kernel<HB>), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    hipLaunchKernelGGL(body::lbs_skin_kp_kernel<HB>, dim3((R + HB - 1) / HB), dim3(256), lds, (hipStream_t)stream, workspace, v_template, v_shapedirs,
                       v_posedirs, v_weights, regressor, verts, keypoints, R, J, nb, NV, VP, NK, scale);
    return check_launch("lbs_skin_kp_kernel");
}

extern "C" int mhe_lbs_skin_err_f32(const float *workspace, const float *v_template, const float *v_shapedirs, const float *v_posedirs,
                                    const float *v_weights, const float *target_verts, const float *center, float *err, int R, int B, int J, int nb,
                                    int NV, int VP, float scale, void *stream) {
    MHE_REQUIRE(workspace && v_template && v_shapedirs && v_posedirs && v_weights && target_verts && err,
                "mhe_lbs_skin_err_f32: null pointer (only center may be null)");
    MHE_REQUIRE(R > 0 && J > 0 && J <= body::MAXJ && nb > 0 && NV > 0 && VP >= NV, "mhe_lbs_skin_err_f32: R=%d J=%d nb=%d NV=%d VP=%d", R, J, nb, NV, VP);
    MHE_REQUIRE(B > 0 && R % B == 0, "mhe_lbs_skin_err_f32: R=%d is not a multiple of B=%d", R, B);
    constexpr int HB = 8;
    hipLaunchKernelGGL(body::lbs_skin_err_kernel<HB>, dim3((R + HB - 1) / HB), dim3(256), 0, (hipStream_t)stream, workspace, v_template, v_shapedirs,
                       v_posedirs, v_weights, target_verts, center, err, R, J, nb, NV, VP, R / B, scale);
    return check_launch("lbs_skin_err_kernel");
}
