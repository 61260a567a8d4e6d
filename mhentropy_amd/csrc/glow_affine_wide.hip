// The ActNorm + LU re-parameterisation of the conditional Glow for a WIDE flow variable (the 144-D body pose; any 2 <= features <= 256).
//
// Same algebra as csrc/glow_affine.hip (formulas there; oracle/glow_ref.py, PARITY UNPINNED), but one float64 matrix at 144 features padded to a
// 192 pitch is 288 KiB - more than a CU's LDS - so the float64 working set lives in a GLOBAL workspace and every phase is its own launch with
// many workgroups per layer (grid.y = layer).  No atomics: every output element is written by one thread, in a fixed order (bit-identical runs).
//   forward:  build L, U, s, shift, diag -> W = L U, A -> c, L^-1, U^-1 (one thread per column: triangular substitution) -> A^-1 = diag(1/s) U^-1 L^-1
//             -> c^-1 = -A^-1 c.  A, c, A^-1, (A^-1)^T, c^-1 leave as f32 zero-padded to the pitch Dp = ceil64(features); const_parts[l] =
//             sum(log_scale) + sum(log diag U).
//   reverse:  dA^-1 [Dp][Dp], dc^-1 [Dp] (f32) and dL/dlog q per row -> float64 gradients of log_scale, shift, lower, upper, unconstrained diagonal
//             and bias, packed per layer [D | D | D(D-1)/2 | D(D-1)/2 | D | D].
#include "common.h"
#include "../../include/mhe.h"

namespace mhe { namespace glowaffw {

constexpr int NT = 256;

__device__ __forceinline__ int low_idx(int i, int j) { return i * (i - 1) / 2 + j; }                               // i > j   (np.tril_indices(D, -1))
__device__ __forceinline__ int up_idx(int i, int j, int D) { return i * (D - 1) - i * (i - 1) / 2 + (j - i - 1); }   // i < j   (np.triu_indices(D, 1))

// per-layer workspace: 9 D x D matrices + 8 vectors of D
//   0 L  1 U  2 W  3 Linv  4 Uinv  5 Ainv  6 G  7 T  8 dA        vectors: s shift diag udiag c dc S(1) -
struct WS {
    double *m[9];
    double *s, *sh, *dg, *ud, *c, *dc, *S;
};
__host__ __device__ __forceinline__ size_t ws_doubles(int D) { return (size_t)9 * D * D + 8 * D; }
__device__ __forceinline__ WS ws_at(double *base, int l, int D) {
    WS w;
    double *p = base + (size_t)l * ws_doubles(D);
    for (int i = 0; i < 9; ++i) w.m[i] = p + (size_t)i * D * D;
    double *v = p + (size_t)9 * D * D;
    w.s = v; w.sh = v + D; w.dg = v + 2 * D; w.ud = v + 3 * D; w.c = v + 4 * D; w.dc = v + 5 * D; w.S = v + 6 * D;
    return w;
}
struct Ptrs { const float *p[6]; };           // log_scale, shift, lower_entries, upper_entries, unconstrained_upper_diag, bias

// ---- forward ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void build_kernel(const Ptrs *__restrict__ params, int D, double eps, double *__restrict__ ws, float *__restrict__ const_parts) {
    const int l = blockIdx.y;
    const Ptrs P = params[l];
    WS w = ws_at(ws, l, D);
    const int i = blockIdx.x * NT + threadIdx.x;
    if (i < D * D) {
        const int r = i / D, k = i % D;
        double u;
        if (r < k) u = (double)P.p[3][up_idx(r, k, D)];
        else if (r == k) { const double ud = (double)P.p[4][r]; u = (ud > 30.0 ? ud : log1p(exp(ud))) + eps; }   // softplus + eps
        else u = 0.0;
        w.m[0][i] = r == k ? 1.0 : r > k ? (double)P.p[2][low_idx(r, k)] : 0.0;
        w.m[1][i] = u;
    }
    if (i < D) {
        const double ud = (double)P.p[4][i];
        w.dg[i] = (ud > 30.0 ? ud : log1p(exp(ud))) + eps;
        w.ud[i] = ud; w.s[i] = exp((double)P.p[0][i]); w.sh[i] = (double)P.p[1][i];
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {              // the log-det constant, summed in index order
        double a = 0.0;
        for (int k = 0; k < D; ++k) {
            const double ud = (double)P.p[4][k];
            a += (double)P.p[0][k] + log((ud > 30.0 ? ud : log1p(exp(ud))) + eps);
        }
        const_parts[l] = (float)a;
    }
}

// W = L U, and A = W diag(s) as f32 [Dp][Dp]
__global__ __launch_bounds__(NT) void lu_product_kernel(int D, int Dp, double *__restrict__ ws, float *__restrict__ A) {
    const int l = blockIdx.y;
    WS w = ws_at(ws, l, D);
    const int i = blockIdx.x * NT + threadIdx.x;
    if (i >= Dp * Dp) return;
    const int r = i / Dp, k = i % Dp;
    float out = 0.f;
    if (r < D && k < D) {
        const double *Lm = w.m[0], *U = w.m[1];
        double a = 0.0;
        const int kmax = r < k ? r : k;                     // L[r][m] = 0 for m > r, U[m][k] = 0 for m > k
        for (int m = 0; m <= kmax; ++m) a = fma(Lm[r * D + m], U[m * D + k], a);
        w.m[2][r * D + k] = a;
        out = (float)(a * w.s[k]);
    }
    A[(size_t)l * Dp * Dp + i] = out;
}

// blockIdx.x = 0: L^-1 (thread = column), 1: U^-1 (thread = column), 2: c = W shift + bias (thread = row)
__global__ __launch_bounds__(NT) void tri_inverse_kernel(const Ptrs *__restrict__ params, int D, double *__restrict__ ws) {
    const int l = blockIdx.y, j = threadIdx.x;
    WS w = ws_at(ws, l, D);
    if (j >= D) return;
    if (blockIdx.x == 0) {
        const double *Lm = w.m[0];
        double *Y = w.m[3];
        for (int i = 0; i < D; ++i) Y[i * D + j] = i == j ? 1.0 : 0.0;
        for (int i = j + 1; i < D; ++i) {
            double a = 0.0;
            for (int k = j; k < i; ++k) a = fma(Lm[i * D + k], Y[k * D + j], a);
            Y[i * D + j] = -a;
        }
    } else if (blockIdx.x == 1) {
        const double *U = w.m[1];
        double *X = w.m[4];
        for (int i = 0; i < D; ++i) X[i * D + j] = 0.0;
        X[j * D + j] = 1.0 / U[j * D + j];
        for (int i = j - 1; i >= 0; --i) {
            double a = 0.0;
            for (int k = i + 1; k <= j; ++k) a = fma(U[i * D + k], X[k * D + j], a);
            X[i * D + j] = -a / U[i * D + i];
        }
    } else {
        double a = (double)params[l].p[5][j];
        for (int k = 0; k < D; ++k) a = fma(w.m[2][j * D + k], w.sh[k], a);
        w.c[j] = a;
    }
}

// A^-1 = diag(1/s) U^-1 L^-1 (f64 kept) -> f32 A^-1 and its transpose [Dp][Dp]
__global__ __launch_bounds__(NT) void ainv_kernel(int D, int Dp, double *__restrict__ ws, float *__restrict__ Ainv, float *__restrict__ AinvT) {
    const int l = blockIdx.y;
    WS w = ws_at(ws, l, D);
    const int i = blockIdx.x * NT + threadIdx.x;
    if (i >= Dp * Dp) return;
    const int r = i / Dp, k = i % Dp;
    float out = 0.f;
    if (r < D && k < D) {
        const double *X = w.m[4], *Y = w.m[3];
        double a = 0.0;
        const int m0 = r > k ? r : k;                       // U^-1[r][m] = 0 for m < r, L^-1[m][k] = 0 for m < k
        for (int m = m0; m < D; ++m) a = fma(X[r * D + m], Y[m * D + k], a);
        a /= w.s[r];
        w.m[5][r * D + k] = a;
        out = (float)a;
    }
    Ainv[(size_t)l * Dp * Dp + i] = out;
    AinvT[(size_t)l * Dp * Dp + (size_t)k * Dp + r] = out;
}

// c (f32) and c^-1 = -A^-1 c
__global__ __launch_bounds__(NT) void cinv_kernel(int D, int Dp, double *__restrict__ ws, float *__restrict__ c_out, float *__restrict__ cinv) {
    const int l = blockIdx.y, r = threadIdx.x;
    WS w = ws_at(ws, l, D);
    if (r >= Dp) return;
    double a = 0.0;
    if (r < D) for (int k = 0; k < D; ++k) a = fma(w.m[5][r * D + k], w.c[k], a);
    cinv[(size_t)l * Dp + r] = r < D ? (float)(-a) : 0.f;
    c_out[(size_t)l * Dp + r] = r < D ? (float)w.c[r] : 0.f;
}

// ---- reverse ---------------------------------------------------------------------------------------------------------------------------
// G = dA^-1 - dc^-1 c^T (c^-1 = -A^-1 c); thread 0 of block 0 also sums S = sum_r dL/dlog q[r] in row order
__global__ __launch_bounds__(NT) void bwd_g_kernel(const float *__restrict__ g_ainv, const float *__restrict__ g_cinv, const float *__restrict__ g_logq,
                                                   long n_logq, int D, int Dp, double *__restrict__ ws) {
    const int l = blockIdx.y;
    WS w = ws_at(ws, l, D);
    const int i = blockIdx.x * NT + threadIdx.x;
    if (i < D * D) {
        const int r = i / D, k = i % D;
        w.m[6][i] = (double)g_ainv[(size_t)l * Dp * Dp + (size_t)r * Dp + k] - (double)g_cinv[(size_t)l * Dp + r] * w.c[k];
    }
    if (i == 0) {
        double s = 0.0;
        for (long q = 0; q < n_logq; ++q) s += (double)g_logq[q];
        w.S[0] = s;
    }
}

// dc = -A^-T dc^-1 (thread = row)
__global__ __launch_bounds__(NT) void bwd_dc_kernel(const float *__restrict__ g_cinv, int D, int Dp, double *__restrict__ ws) {
    const int l = blockIdx.y, t = threadIdx.x;
    WS w = ws_at(ws, l, D);
    if (t >= D) return;
    double a = 0.0;
    for (int k = 0; k < D; ++k) a = fma(w.m[5][k * D + t], (double)g_cinv[(size_t)l * Dp + k], a);
    w.dc[t] = -a;
}

// T = A^-T G
__global__ __launch_bounds__(NT) void bwd_t_kernel(int D, double *__restrict__ ws) {
    const int l = blockIdx.y;
    WS w = ws_at(ws, l, D);
    const int i = blockIdx.x * NT + threadIdx.x;
    if (i >= D * D) return;
    const int r = i / D, k = i % D;
    const double *Ai = w.m[5], *G = w.m[6];
    double a = 0.0;
    for (int m = 0; m < D; ++m) a = fma(Ai[m * D + r], G[m * D + k], a);
    w.m[7][i] = a;
}

// dA = -T A^-T;  dW = dA diag(s) + dc shift^T  (dW overwrites G)
__global__ __launch_bounds__(NT) void bwd_da_kernel(int D, double *__restrict__ ws) {
    const int l = blockIdx.y;
    WS w = ws_at(ws, l, D);
    const int i = blockIdx.x * NT + threadIdx.x;
    if (i >= D * D) return;
    const int r = i / D, k = i % D;
    const double *Ai = w.m[5], *T = w.m[7];
    double a = 0.0;
    for (int m = 0; m < D; ++m) a = fma(T[r * D + m], Ai[k * D + m], a);
    w.m[8][i] = -a;
    w.m[6][i] = -a * w.s[k] + w.dc[r] * w.sh[k];
}

// per layer output [log_scale D | shift D | lower n | upper n | udiag D | bias D], n = D (D - 1) / 2
__host__ __device__ __forceinline__ size_t grad_stride(int D) { return (size_t)4 * D + (size_t)D * (D - 1); }

// dlog_scale = colsum(dA o W) s + S;  dshift = W^T dc;  dbias = dc   (thread = column)
__global__ __launch_bounds__(NT) void bwd_vec_kernel(int D, double *__restrict__ ws, double *__restrict__ grads) {
    const int l = blockIdx.y, t = threadIdx.x;
    WS w = ws_at(ws, l, D);
    if (t >= D) return;
    const double *dA = w.m[8], *W = w.m[2];
    double a = 0.0, b = 0.0;
    for (int m = 0; m < D; ++m) { a = fma(dA[m * D + t], W[m * D + t], a); b = fma(W[m * D + t], w.dc[m], b); }
    double *g = grads + (size_t)l * grad_stride(D);
    const size_t n = (size_t)D * (D - 1) / 2;
    g[t] = a * w.s[t] + w.S[0];
    g[D + t] = b;
    g[3 * D + 2 * n + t] = w.dc[t];
}

// dL = dW U^T (strict lower), dU = L^T dW (upper), dudiag = (diag(dU) + S / diag) sigmoid(udiag)
__global__ __launch_bounds__(NT) void bwd_lu_kernel(int D, double *__restrict__ ws, double *__restrict__ grads) {
    const int l = blockIdx.y;
    WS w = ws_at(ws, l, D);
    const int i = blockIdx.x * NT + threadIdx.x;
    if (i >= D * D) return;
    const int r = i / D, k = i % D;
    const double *dW = w.m[6], *Lm = w.m[0], *U = w.m[1];
    double *g = grads + (size_t)l * grad_stride(D);
    const size_t n = (size_t)D * (D - 1) / 2;
    if (r > k) {
        double a = 0.0;
        for (int m = k; m < D; ++m) a = fma(dW[r * D + m], U[k * D + m], a);              // U[k][m] = 0 for m < k
        g[2 * D + low_idx(r, k)] = a;
    } else {
        double a = 0.0;
        for (int m = r; m < D; ++m) a = fma(Lm[m * D + r], dW[m * D + k], a);             // L[m][r] = 0 for m < r
        if (r < k) g[2 * D + n + up_idx(r, k, D)] = a;
        else g[2 * D + 2 * n + r] = (a + w.S[0] / w.dg[r]) / (1.0 + exp(-w.ud[r]));
    }
}

// ---- reverse of the DENSITY direction ---------------------------------------------------------------------------------------------------
// v = A u + c is applied as it stands, so the gradients arrive on A and c themselves (formulas: csrc/glow_affine.hip, density_bwd_kernel):
// dA (f64 copy) -> slot 8, dW = dA diag(s) + dc shift^T -> slot 6, dc -> its vector, S = sum_r dL/dlog p[r] (block 0: strided partial sums, then a
// tree over the 256 threads - a fixed order); bwd_vec_kernel and bwd_lu_kernel then finish exactly as for the sampling direction.
__global__ __launch_bounds__(NT) void bwd_density_kernel(const float *__restrict__ g_a, const float *__restrict__ g_c, const float *__restrict__ g_logp,
                                                         long n_logp, int D, int Dp, double *__restrict__ ws) {
    __shared__ double red[NT];
    const int l = blockIdx.y, tid = threadIdx.x;
    WS w = ws_at(ws, l, D);
    const int i = blockIdx.x * NT + tid;
    if (i < D * D) {
        const int r = i / D, k = i % D;
        const double a = (double)g_a[(size_t)l * Dp * Dp + (size_t)r * Dp + k];
        w.m[8][i] = a;
        w.m[6][i] = a * w.s[k] + (double)g_c[(size_t)l * Dp + r] * w.sh[k];
    }
    if (blockIdx.x == 0) {
        if (tid < D) w.dc[tid] = (double)g_c[(size_t)l * Dp + tid];
        double s = 0.0;
        for (long q = tid; q < n_logp; q += NT) s += (double)g_logp[q];
        red[tid] = s;
        __syncthreads();
        for (int o = NT / 2; o > 0; o >>= 1) { if (tid < o) red[tid] += red[tid + o]; __syncthreads(); }
        if (tid == 0) w.S[0] = red[0];
    }
}

}}  // namespace mhe::glowaffw

using namespace mhe;

static inline int pad64(int n) { return (n + 63) / 64 * 64; }

extern "C" size_t mhe_glow_affine_wide_workspace_doubles(int layers, int features) {
    return layers > 0 && features > 1 && features <= 256 ? (size_t)layers * glowaffw::ws_doubles(features) : 0;
}

extern "C" size_t mhe_glow_affine_wide_grad_doubles(int layers, int features) {
    return layers > 0 && features > 1 && features <= 256 ? (size_t)layers * glowaffw::grad_stride(features) : 0;
}

extern "C" int mhe_glow_affine_wide_f64(const void *param_ptrs, int layers, int features, double eps, float *A, float *c, float *Ainv, float *AinvT,
                                        float *cinv, float *const_parts, double *workspace, void *stream) {
    MHE_REQUIRE(layers > 0 && layers <= 65535 && features > 1 && features <= 256, "mhe_glow_affine_wide_f64: features=%d (2..256), layers=%d", features, layers);
    MHE_REQUIRE(on_device(param_ptrs) && on_device(A) && on_device(c) && on_device(Ainv) && on_device(AinvT) && on_device(cinv) && on_device(const_parts) &&
                    on_device(workspace), "mhe_glow_affine_wide_f64: every buffer must be device memory");
    const int D = features, Dp = pad64(D);
    hipStream_t s = (hipStream_t)stream;
    const glowaffw::Ptrs *P = (const glowaffw::Ptrs *)param_ptrs;
    const unsigned nd = (unsigned)((D * D + glowaffw::NT - 1) / glowaffw::NT), np = (unsigned)((Dp * Dp + glowaffw::NT - 1) / glowaffw::NT);
    hipLaunchKernelGGL(glowaffw::build_kernel, dim3(nd, layers), dim3(glowaffw::NT), 0, s, P, D, eps, workspace, const_parts);
    hipLaunchKernelGGL(glowaffw::lu_product_kernel, dim3(np, layers), dim3(glowaffw::NT), 0, s, D, Dp, workspace, A);
    hipLaunchKernelGGL(glowaffw::tri_inverse_kernel, dim3(3, layers), dim3(glowaffw::NT), 0, s, P, D, workspace);
    hipLaunchKernelGGL(glowaffw::ainv_kernel, dim3(np, layers), dim3(glowaffw::NT), 0, s, D, Dp, workspace, Ainv, AinvT);
    hipLaunchKernelGGL(glowaffw::cinv_kernel, dim3(1, layers), dim3(glowaffw::NT), 0, s, D, Dp, workspace, c, cinv);
    return check_launch("glowaffw::affine");
}

extern "C" int mhe_glow_affine_wide_bwd_f64(const float *g_ainv, const float *g_cinv, const float *g_log_q, long n_log_q, int layers, int features,
                                            double *workspace, double *grads, void *stream) {
    MHE_REQUIRE(layers > 0 && layers <= 65535 && features > 1 && features <= 256 && n_log_q >= 0 && (n_log_q == 0 || g_log_q),
                "mhe_glow_affine_wide_bwd_f64: features=%d (2..256), layers=%d, n_log_q=%ld", features, layers, n_log_q);
    MHE_REQUIRE(on_device(g_ainv) && on_device(g_cinv) && on_device(workspace) && on_device(grads) && (n_log_q == 0 || on_device(g_log_q)),
                "mhe_glow_affine_wide_bwd_f64: every buffer must be device memory");
    const int D = features, Dp = pad64(D);
    hipStream_t s = (hipStream_t)stream;
    const unsigned nd = (unsigned)((D * D + glowaffw::NT - 1) / glowaffw::NT);
    hipLaunchKernelGGL(glowaffw::bwd_g_kernel, dim3(nd, layers), dim3(glowaffw::NT), 0, s, g_ainv, g_cinv, g_log_q, n_log_q, D, Dp, workspace);
    hipLaunchKernelGGL(glowaffw::bwd_dc_kernel, dim3(1, layers), dim3(glowaffw::NT), 0, s, g_cinv, D, Dp, workspace);
    hipLaunchKernelGGL(glowaffw::bwd_t_kernel, dim3(nd, layers), dim3(glowaffw::NT), 0, s, D, workspace);
    hipLaunchKernelGGL(glowaffw::bwd_da_kernel, dim3(nd, layers), dim3(glowaffw::NT), 0, s, D, workspace);
    hipLaunchKernelGGL(glowaffw::bwd_vec_kernel, dim3(1, layers), dim3(glowaffw::NT), 0, s, D, workspace, grads);
    hipLaunchKernelGGL(glowaffw::bwd_lu_kernel, dim3(nd, layers), dim3(glowaffw::NT), 0, s, D, workspace, grads);
    return check_launch("glowaffw::reparam_bwd");
}

extern "C" int mhe_glow_affine_wide_density_bwd_f64(const float *g_a, const float *g_c, const float *g_log_p, long n_log_p, int layers, int features,
                                                    double *workspace, double *grads, void *stream) {
    MHE_REQUIRE(layers > 0 && layers <= 65535 && features > 1 && features <= 256 && n_log_p >= 0 && (n_log_p == 0 || g_log_p),
                "mhe_glow_affine_wide_density_bwd_f64: features=%d (2..256), layers=%d, n_log_p=%ld", features, layers, n_log_p);
    MHE_REQUIRE(on_device(g_a) && on_device(g_c) && on_device(workspace) && on_device(grads) && (n_log_p == 0 || on_device(g_log_p)),
                "mhe_glow_affine_wide_density_bwd_f64: every buffer must be device memory");
    const int D = features, Dp = pad64(D);
    hipStream_t s = (hipStream_t)stream;
    const unsigned nd = (unsigned)((D * D + glowaffw::NT - 1) / glowaffw::NT);
    hipLaunchKernelGGL(glowaffw::bwd_density_kernel, dim3(nd, layers), dim3(glowaffw::NT), 0, s, g_a, g_c, n_log_p ? g_log_p : nullptr, n_log_p, D, Dp,
                       workspace);
    hipLaunchKernelGGL(glowaffw::bwd_vec_kernel, dim3(1, layers), dim3(glowaffw::NT), 0, s, D, workspace, grads);
    hipLaunchKernelGGL(glowaffw::bwd_lu_kernel, dim3(nd, layers), dim3(glowaffw::NT), 0, s, D, workspace, grads);
    return check_launch("glowaffw::density_bwd");
}
