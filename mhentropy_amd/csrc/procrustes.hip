// Procrustes alignment with scale of every hypothesis to its image's ground truth: the aligned branch of MHEntLoss
// (hand/criteria.py:62-87) around align_w_scale (hand/utils.py:502-525) and scipy.linalg.orthogonal_procrustes.  Per row
// (n, b), A = target[b] and Bm = pred[n, b], both P x 3:
//   t1 = mean(A), A0 = (A - t1) / s1, s1 = |A - t1|_F + 1e-8;   t2 = mean(Bm), B0 = (Bm - t2) / s2, s2 = |Bm - t2|_F + 1e-8
//   M = A0^T B0 = U S V^T,  R = U V^T (no determinant correction: reflections are kept),  s = trace(S)
//   out = (B0 R^T) * s * s1 + t1
// Three launches' worth of structure in two kernels and a shared 3x3 step:
//   target_kernel   once per IMAGE: t1, s1 (f64 sums) and the centred, scaled rows A0 into the workspace;
//   rows_kernel     P <= 32 (the 21 joints): one THREAD per hypothesis.  A workgroup stages up to 256 rows of one image by
//                   coalesced loads into LDS, every thread reduces its own row and takes its own polar factor, writes the
//                   aligned row back in place, and the workgroup stores the chunk coalesced;
//   wave_kernel     larger P (the 778-vertex mesh): one WAVE per hypothesis, the row read from HBM once into the wave's LDS
//                   slice, point sums over the lanes, the polar factor in every lane, the aligned row written back through LDS.
// M is accumulated from CENTRED rows in f32 (targets sit ~0.5 m from the origin at a ~0.1 m extent: the uncentred form would
// cancel); the polar factor is taken in f64 by Jacobi on M^T M, U = M V S^-1 by Gram-Schmidt, which keeps det(R) = det(U) det(V)
// of whatever sign M has and stays finite when M is singular (M = 0: s = 0, out = t1 exactly).
#include "common.h"

namespace mhe { namespace procrustes {

constexpr int PMAX = 1024;          // points per row the wave kernel's LDS slices are sized for
constexpr int PSMALL = 32;          // rows_kernel up to here
constexpr int CH = 256;             // rows_kernel: hypotheses per workgroup
constexpr int WAVES = 4;            // wave_kernel: waves per workgroup
constexpr int HPW = 4;              // wave_kernel: hypotheses per wave

__host__ __device__ inline int ws_stride(int P) { return (P * 3 + 4 + 1) & ~1; }     // A0 [P*3], t1 [3], s1; even (8-byte rows)

// ---- polar factor of a 3x3 matrix ---------------------------------------------------------------------------------------------
// Cyclic Jacobi on the symmetric K = M^T M: K = V diag(lambda) V^T.  Columns sorted by lambda descending, then
// u_i = M v_i orthonormalised in that order (Gram-Schmidt); a column whose remainder is negligible against |M v_1| is completed
// as a unit vector orthogonal to the ones before (u_2) or u_1 x u_2 (u_3).  R = sum_i u_i v_i^T, s = trace(R^T M) = trace(S).
__device__ inline void polar3(const double m[9], double r[9], double &s) {
    double a[3][3], v[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            a[i][j] = m[0 * 3 + i] * m[0 * 3 + j] + m[1 * 3 + i] * m[1 * 3 + j] + m[2 * 3 + i] * m[2 * 3 + j];
            v[i][j] = i == j ? 1.0 : 0.0;
        }
    for (int sweep = 0; sweep < 8; ++sweep) {              // quadratic convergence: 3-4 sweeps
        const double off = a[0][1] * a[0][1] + a[0][2] * a[0][2] + a[1][2] * a[1][2];
        const double dia = a[0][0] * a[0][0] + a[1][1] * a[1][1] + a[2][2] * a[2][2];
        if (!(off > 1e-26 * dia)) break;                    // off-diagonal below 1e-13 of the diagonal; also ends on K = 0 and on NaN
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int p = k == 2 ? 1 : 0, q = k == 0 ? 1 : 2;
            const int o = 3 - p - q;
            const double apq = a[p][q];
            if (apq == 0.0) continue;
            const double th = (a[q][q] - a[p][p]) / (2.0 * apq);
            const double t = fabs(th) > 1e150 ? 0.5 / th : copysign(1.0, th) / (fabs(th) + sqrt(th * th + 1.0));
            const double c = 1.0 / sqrt(t * t + 1.0), sn = t * c;
            a[p][p] -= t * apq;
            a[q][q] += t * apq;
            a[p][q] = a[q][p] = 0.0;
            const double aop = a[o][p], aoq = a[o][q];
            a[o][p] = a[p][o] = c * aop - sn * aoq;
            a[o][q] = a[q][o] = sn * aop + c * aoq;
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const double vp = v[i][p], vq = v[i][q];
                v[i][p] = c * vp - sn * vq;
                v[i][q] = sn * vp + c * vq;
            }
        }
    }
    double lam[3] = {a[0][0], a[1][1], a[2][2]};
    int ord[3] = {0, 1, 2};
    if (lam[ord[0]] < lam[ord[1]]) { const int x = ord[0]; ord[0] = ord[1]; ord[1] = x; }
    if (lam[ord[1]] < lam[ord[2]]) { const int x = ord[1]; ord[1] = ord[2]; ord[2] = x; }
    if (lam[ord[0]] < lam[ord[1]]) { const int x = ord[0]; ord[0] = ord[1]; ord[1] = x; }
    double vc[3][3], u[3][3];                               // vc[i] = v_i, u[i] = u_i (vectors)
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int k = 0; k < 3; ++k) vc[i][k] = ord[i] == 0 ? v[k][0] : (ord[i] == 1 ? v[k][1] : v[k][2]);
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int k = 0; k < 3; ++k) u[i][k] = m[k * 3 + 0] * vc[i][0] + m[k * 3 + 1] * vc[i][1] + m[k * 3 + 2] * vc[i][2];
    const double n1 = sqrt(u[0][0] * u[0][0] + u[0][1] * u[0][1] + u[0][2] * u[0][2]);
    const double tiny = 1e-13 * n1;
    if (n1 > 0.0) {
#pragma unroll
        for (int k = 0; k < 3; ++k) u[0][k] /= n1;
    } else {
        u[0][0] = 1.0; u[0][1] = 0.0; u[0][2] = 0.0;
    }
    {
        const double d = u[1][0] * u[0][0] + u[1][1] * u[0][1] + u[1][2] * u[0][2];
#pragma unroll
        for (int k = 0; k < 3; ++k) u[1][k] -= d * u[0][k];
        const double n2 = sqrt(u[1][0] * u[1][0] + u[1][1] * u[1][1] + u[1][2] * u[1][2]);
        if (n2 > tiny && n2 > 0.0) {
#pragma unroll
            for (int k = 0; k < 3; ++k) u[1][k] /= n2;
        } else {                                            // any unit vector orthogonal to u_1: the axis least along it, projected out
            const double ax = fabs(u[0][0]), ay = fabs(u[0][1]), az = fabs(u[0][2]);
            double e[3] = {0.0, 0.0, 0.0};
            e[(ax <= ay && ax <= az) ? 0 : (ay <= az ? 1 : 2)] = 1.0;
            const double de = e[0] * u[0][0] + e[1] * u[0][1] + e[2] * u[0][2];
#pragma unroll
            for (int k = 0; k < 3; ++k) u[1][k] = e[k] - de * u[0][k];
            const double ne = sqrt(u[1][0] * u[1][0] + u[1][1] * u[1][1] + u[1][2] * u[1][2]);
#pragma unroll
            for (int k = 0; k < 3; ++k) u[1][k] /= ne;
        }
    }
    {
        const double d0 = u[2][0] * u[0][0] + u[2][1] * u[0][1] + u[2][2] * u[0][2];
        const double d1 = u[2][0] * u[1][0] + u[2][1] * u[1][1] + u[2][2] * u[1][2];
#pragma unroll
        for (int k = 0; k < 3; ++k) u[2][k] -= d0 * u[0][k] + d1 * u[1][k];
        const double n3 = sqrt(u[2][0] * u[2][0] + u[2][1] * u[2][1] + u[2][2] * u[2][2]);
        if (n3 > tiny && n3 > 0.0) {
#pragma unroll
            for (int k = 0; k < 3; ++k) u[2][k] /= n3;
        } else {
            u[2][0] = u[0][1] * u[1][2] - u[0][2] * u[1][1];
            u[2][1] = u[0][2] * u[1][0] - u[0][0] * u[1][2];
            u[2][2] = u[0][0] * u[1][1] - u[0][1] * u[1][0];
        }
    }
    s = 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            r[i * 3 + j] = u[0][i] * vc[0][j] + u[1][i] * vc[1][j] + u[2][i] * vc[2][j];
            s += r[i * 3 + j] * m[i * 3 + j];
        }
}

// ---- per-image target statistics: once per image --------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void target_kernel(const float *__restrict__ tgt, float *__restrict__ ws, int P) {
    __shared__ double red[4][4];
    const int b = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const float *a = tgt + (size_t)b * P * 3;
    float *w = ws + (size_t)b * ws_stride(P);
    double sx = 0.0, sy = 0.0, sz = 0.0;
    for (int p = tid; p < P; p += 256) { sx += a[p * 3]; sy += a[p * 3 + 1]; sz += a[p * 3 + 2]; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { sx += __shfl_xor(sx, o, 64); sy += __shfl_xor(sy, o, 64); sz += __shfl_xor(sz, o, 64); }
    if (lane == 0) { red[wave][0] = sx; red[wave][1] = sy; red[wave][2] = sz; }
    __syncthreads();
    const double tx = (red[0][0] + red[1][0] + red[2][0] + red[3][0]) / P;
    const double ty = (red[0][1] + red[1][1] + red[2][1] + red[3][1]) / P;
    const double tz = (red[0][2] + red[1][2] + red[2][2] + red[3][2]) / P;
    const float t1[3] = {(float)tx, (float)ty, (float)tz};          // the f32 mean numpy takes of f32 rows, to rounding
    double q = 0.0;
    for (int p = tid; p < P; p += 256)
#pragma unroll
        for (int d = 0; d < 3; ++d) { const double c = (double)(a[p * 3 + d] - t1[d]); q += c * c; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) q += __shfl_xor(q, o, 64);
    __syncthreads();
    if (lane == 0) red[wave][3] = q;
    __syncthreads();
    const float s1 = (float)sqrt(red[0][3] + red[1][3] + red[2][3] + red[3][3]) + 1e-8f;
    for (int p = tid; p < P; p += 256)
#pragma unroll
        for (int d = 0; d < 3; ++d) w[p * 3 + d] = (a[p * 3 + d] - t1[d]) / s1;
    if (tid == 0) { w[P * 3] = t1[0]; w[P * 3 + 1] = t1[1]; w[P * 3 + 2] = t1[2]; w[P * 3 + 3] = s1; }
}

// M (row-major, M[i][j] = sum_p A0[p][i] B0[p][j]) of the CENTRED, UNSCALED B rows -> R, s; k = s * s1 / s2
__device__ __forceinline__ void solve(const float mr[9], float q, float *rf, float &sf, float &kf, float s1) {
    const float s2 = sqrtf(q) + 1e-8f;
    double m[9], r[9], s;
#pragma unroll
    for (int i = 0; i < 9; ++i) m[i] = (double)mr[i] / (double)s2;
    polar3(m, r, s);
#pragma unroll
    for (int i = 0; i < 9; ++i) rf[i] = (float)r[i];
    sf = (float)s;
    kf = (float)(s * (double)s1 / (double)s2);
}

// ---- P <= PSMALL: one thread per hypothesis ---------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void rows_kernel(const float *__restrict__ pred, const float *__restrict__ ws, float *__restrict__ out,
                                                   float *__restrict__ Rout, float *__restrict__ sout, int N, int B, int P) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int b = blockIdx.y, n0 = blockIdx.x * CH, tid = threadIdx.x, P3 = P * 3;
    float *a0 = lds, *buf = lds + ws_stride(P);             // A0, t1, s1 of image b; then [cn][P3] hypothesis rows
    const int cn = N - n0 < CH ? N - n0 : CH;
    const float *w = ws + (size_t)b * ws_stride(P);
    for (int i = tid; i < P3 + 4; i += 256) a0[i] = w[i];
    for (int i = tid; i < cn * P3; i += 256) {
        const int n = i / P3, j = i - n * P3;
        buf[n * P3 + j] = pred[((size_t)(n0 + n) * B + b) * P3 + j];
    }
    __syncthreads();
    if (tid < cn) {
        float *c = buf + tid * P3;                          // row stride P3: odd for P = 21, conflict-free
        float t2[3] = {0.f, 0.f, 0.f};
        for (int p = 0; p < P; ++p)
#pragma unroll
            for (int d = 0; d < 3; ++d) t2[d] += c[p * 3 + d];
#pragma unroll
        for (int d = 0; d < 3; ++d) t2[d] /= (float)P;
        float q = 0.f, mr[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        for (int p = 0; p < P; ++p) {
            const float x[3] = {c[p * 3] - t2[0], c[p * 3 + 1] - t2[1], c[p * 3 + 2] - t2[2]};
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                q = fmaf(x[i], x[i], q);
                const float ai = a0[p * 3 + i];
#pragma unroll
                for (int j = 0; j < 3; ++j) mr[i * 3 + j] = fmaf(ai, x[j], mr[i * 3 + j]);
            }
        }
        float r[9], s, k;
        solve(mr, q, r, s, k, a0[P3 + 3]);
        for (int p = 0; p < P; ++p) {
            const float x[3] = {c[p * 3] - t2[0], c[p * 3 + 1] - t2[1], c[p * 3 + 2] - t2[2]};
#pragma unroll
            for (int i = 0; i < 3; ++i) c[p * 3 + i] = fmaf(r[i * 3] * x[0] + r[i * 3 + 1] * x[1] + r[i * 3 + 2] * x[2], k, a0[P3 + i]);
        }
        const size_t row = (size_t)(n0 + tid) * B + b;
        if (Rout)
#pragma unroll
            for (int i = 0; i < 9; ++i) Rout[row * 9 + i] = r[i];
        if (sout) sout[row] = s;
    }
    __syncthreads();
    for (int i = tid; i < cn * P3; i += 256) {
        const int n = i / P3, j = i - n * P3;
        out[((size_t)(n0 + n) * B + b) * P3 + j] = buf[n * P3 + j];
    }
}

// ---- larger P: one wave per hypothesis ----------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void wave_kernel(const float *__restrict__ pred, const float *__restrict__ ws, float *__restrict__ out,
                                                   float *__restrict__ Rout, float *__restrict__ sout, int N, int B, int P) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int b = blockIdx.y, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, P3 = P * 3, S = ws_stride(P);
    float *a0 = lds;                                        // [S]: A0, t1, s1 of image b
    float *buf = lds + S + wave * S;                        // this wave's row
    const float *w = ws + (size_t)b * S;
    for (int i = tid; i < P3 + 4; i += 256) a0[i] = w[i];
    __syncthreads();
    const float t1[3] = {a0[P3], a0[P3 + 1], a0[P3 + 2]}, s1 = a0[P3 + 3];
    const bool vec = ((P3 & 1) == 0) && ((reinterpret_cast<size_t>(pred) | reinterpret_cast<size_t>(out)) & 7) == 0;
    for (int h = 0; h < HPW; ++h) {
        const int n = (blockIdx.x * WAVES + wave) * HPW + h;
        if (n >= N) break;
        const size_t row = (size_t)n * B + b;
        const float *src = pred + row * P3;
        if (vec) {
            const float2 *s2p = reinterpret_cast<const float2 *>(src);
            float2 *d2 = reinterpret_cast<float2 *>(buf);
#pragma unroll 4
            for (int i = lane; i < P3 / 2; i += 64) d2[i] = s2p[i];
        } else {
            for (int i = lane; i < P3; i += 64) buf[i] = src[i];
        }
        wave_sync();
        float t2[3] = {0.f, 0.f, 0.f};
        for (int p = lane; p < P; p += 64)
#pragma unroll
            for (int d = 0; d < 3; ++d) t2[d] += buf[p * 3 + d];
#pragma unroll
        for (int d = 0; d < 3; ++d) t2[d] = wave_sum(t2[d]) / (float)P;
        float q = 0.f, mr[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        for (int p = lane; p < P; p += 64) {
            const float x[3] = {buf[p * 3] - t2[0], buf[p * 3 + 1] - t2[1], buf[p * 3 + 2] - t2[2]};
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                q = fmaf(x[i], x[i], q);
                const float ai = a0[p * 3 + i];
#pragma unroll
                for (int j = 0; j < 3; ++j) mr[i * 3 + j] = fmaf(ai, x[j], mr[i * 3 + j]);
            }
        }
        q = wave_sum(q);
#pragma unroll
        for (int i = 0; i < 9; ++i) mr[i] = wave_sum(mr[i]);        // xor butterflies: every lane holds the same bits
        float r[9], s, k;
        solve(mr, q, r, s, k, s1);
        for (int p = lane; p < P; p += 64) {
            const float x[3] = {buf[p * 3] - t2[0], buf[p * 3 + 1] - t2[1], buf[p * 3 + 2] - t2[2]};
#pragma unroll
            for (int i = 0; i < 3; ++i) buf[p * 3 + i] = fmaf(r[i * 3] * x[0] + r[i * 3 + 1] * x[1] + r[i * 3 + 2] * x[2], k, t1[i]);
        }
        wave_sync();
        float *dst = out + row * P3;
        if (vec) {
            float2 *d2 = reinterpret_cast<float2 *>(dst);
            const float2 *b2 = reinterpret_cast<const float2 *>(buf);
#pragma unroll 4
            for (int i = lane; i < P3 / 2; i += 64) d2[i] = b2[i];
        } else {
            for (int i = lane; i < P3; i += 64) dst[i] = buf[i];
        }
        if (Rout && lane < 9) Rout[row * 9 + lane] = r[lane];
        if (sout && lane == 0) sout[row] = s;
        wave_sync();                                        // the next row's loads overwrite buf
    }
}

}}  // namespace mhe::procrustes

using namespace mhe;

extern "C" size_t mhe_procrustes_workspace_floats(int B, int P) {
    return B > 0 && P > 0 ? (size_t)B * procrustes::ws_stride(P) : 0;
}

extern "C" int mhe_procrustes_align_f32(const float *pred, const float *target, float *out, float *R, float *s, float *ws,
                                        size_t ws_floats, int N, int B, int P, void *stream) {
    using namespace procrustes;
    MHE_REQUIRE(pred && target && out && ws, "mhe_procrustes_align_f32: null pointer");
    MHE_REQUIRE(N > 0 && B > 0 && B <= 65535 && P > 0 && P <= PMAX, "mhe_procrustes_align_f32: need N > 0, 0 < B <= 65535, 0 < P <= %d "
                "(N=%d B=%d P=%d)", PMAX, N, B, P);
    MHE_REQUIRE(ws_floats >= mhe_procrustes_workspace_floats(B, P), "mhe_procrustes_align_f32: workspace of %zu floats, need %zu", ws_floats,
                mhe_procrustes_workspace_floats(B, P));
    MHE_REQUIRE(on_device(pred) && on_device(target) && on_device(out) && on_device(ws) && (!R || on_device(R)) && (!s || on_device(s)),
                "mhe_procrustes_align_f32: every pointer must be device memory");
    const size_t rows = (size_t)N * B, f = sizeof(float);
    const size_t np = rows * P * 3 * f, nt = (size_t)B * P * 3 * f, nw = ws_floats * f, nr = rows * 9 * f, ns = rows * f;
    MHE_REQUIRE(disjoint(out, np, pred, np) && disjoint(out, np, target, nt) && disjoint(out, np, ws, nw) && disjoint(ws, nw, pred, np) &&
                disjoint(ws, nw, target, nt) && disjoint(R, nr, pred, np) && disjoint(R, nr, target, nt) && disjoint(R, nr, out, np) &&
                disjoint(R, nr, ws, nw) && disjoint(s, ns, pred, np) && disjoint(s, ns, target, nt) && disjoint(s, ns, out, np) &&
                disjoint(s, ns, ws, nw) && disjoint(R, nr, s, ns),
                "mhe_procrustes_align_f32: out, R, s and ws must not overlap each other or the inputs");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(target_kernel, dim3(B), dim3(256), 0, st, target, ws, P);
    if (int e = check_launch("procrustes target_kernel")) return e;
    static const bool set = [] {
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(rows_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (ws_stride(PSMALL) + CH * PSMALL * 3) * (int)sizeof(float));
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(wave_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (1 + WAVES) * ws_stride(PMAX) * (int)sizeof(float));
        return true;
    }();
    (void)set;
    if (P <= PSMALL) {
        const int lds = (ws_stride(P) + CH * P * 3) * (int)sizeof(float);
        hipLaunchKernelGGL(rows_kernel, dim3((N + CH - 1) / CH, B), dim3(256), lds, st, pred, ws, out, R, s, N, B, P);
        return check_launch("procrustes rows_kernel");
    }
    const int lds = (1 + WAVES) * ws_stride(P) * (int)sizeof(float);
    hipLaunchKernelGGL(wave_kernel, dim3((N + WAVES * HPW - 1) / (WAVES * HPW), B), dim3(256), lds, st, pred, ws, out, R, s, N, B, P);
    return check_launch("procrustes wave_kernel");
}
