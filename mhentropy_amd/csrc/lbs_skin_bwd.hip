// Reverse of the body model's vertex skinning (lbs_skin_mfma_kernel, csrc/lbs_skin.hip; the arithmetic of hand/manopth/manolayer.py:181-246 at
// runtime sizes) on the matrix cores in EXACT f32: v_mfma_f32_32x32x2_f32 (one f32 per lane and operand, a k-ordered fmaf chain per output).
// With x_v = vt_v + SD_v beta + PD_v p, h_v = [x_v; 1], T_v = sum_j w_vj A_j (A_j = [Rw_j | a_j], the workspace row of lbs_pose_kernel) and
// vert_v = scale T_v h_v, an incoming g_v = dL/dvert_v gives u_v = scale g_v and
//   g_A_j = sum_v w_vj u_v h_v^T                          (kernel A: lbs_skin_bwd_tf_kernel, the forward's blend product X recomputed)
//   g_x_v = T_v[:, :3]^T u_v;  [g_p | g_beta] = sum_v [PD_v | SD_v]^T g_x_v   (kernel G: lbs_skin_bwd_coef_kernel, the rotation part of T recomputed)
// Both are reductions over the vertices: vertex = k of the MFMA, hypothesis = row (32 per workgroup, A operands from LDS), coefficient / joint =
// column (B operands: coefficient-fastest tables made once per model by mhe_lbs_bwd_tables_f32).  Per 32-vertex tile a wave recomputes what the
// forward had in the accumulator layout (vertex = lane), forms g_x / u / x lane-locally, and moves them through a wave-private LDS image into
// A-operand layout (vertex = k).  Each wave keeps its own accumulators over the tiles it visits (wave w: tiles w, w + 4, ...); the four waves'
// partials are summed in a fixed order at the end.  No atomics: two calls give bit-identical results.  The pose chain's reverse is in body.hip
// (mhe_lbs_transforms_bwd_f32).
#include "common.h"

namespace mhe { namespace body {

// workspace row of lbs_pose_kernel (body.hip): pose map [9(J-1)] | betas [nb] | skinning transforms [J][12] | posed joints [J][3]
__host__ __device__ inline int sbw_stride(int J, int nb) { return (9 * (J - 1) + nb + 15 * J + 15) / 16 * 16; }
// coefficient columns of kernel G: pose map then betas, padded to whole 32-column tiles
__host__ __device__ inline int sbw_nt(int J, int nb) { return (9 * (J - 1) + nb + 31) / 32; }
// the reverse's tables: PDT [VP][3][32 NT] (row = (vertex, coordinate), column = coefficient), then WT [VP][32] (column = joint)
__host__ __device__ inline size_t sbw_tables_floats(int J, int nb, int VP) { return (size_t)VP * 3 * 32 * sbw_nt(J, nb) + (size_t)VP * 32; }
__host__ __device__ inline size_t sbw_lds_g(int J) { return ((size_t)9 * ((J + 1) / 2 * 2) * 32 + 4 * 96 * 33) * 4; }
__host__ __device__ inline size_t sbw_lds_a(int J, int nb) { return ((size_t)(9 * (J - 1) + nb + 1) / 2 * 2 * 32 + 4 * 6 * 32 * 33) * 4; }

typedef __attribute__((ext_vector_type(16))) float f32x16;
#define MFMA32(a, b, c) c = __builtin_amdgcn_mfma_f32_32x32x2f32((a), (b), (c), 0, 0, 0)

__device__ __forceinline__ int acc_row(int i, int half) { return (i & 3) + 8 * (i >> 2) + 4 * half; }

__global__ __launch_bounds__(256) void lbs_bwd_tables_kernel(const float *__restrict__ Vsd, const float *__restrict__ Vpd,
                                                             const float *__restrict__ Vw, float *__restrict__ out, int J, int nb, int NV, int VP) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    const int NP = 9 * (J - 1), NC = NP + nb, NCP = 32 * sbw_nt(J, nb);
    const long npd = (long)VP * 3 * NCP;
    if (t < npd) {
        const int k = (int)(t % NCP);
        const long rc = t / NCP;
        const int c = (int)(rc % 3), v = (int)(rc / 3);
        float x = 0.f;
        if (v < NV && k < NC) x = k < NP ? Vpd[((size_t)k * 3 + c) * VP + v] : Vsd[((size_t)(k - NP) * 3 + c) * VP + v];
        out[t] = x;
    } else if (t < npd + (long)VP * 32) {
        const long q = t - npd;
        const int j = (int)(q & 31), v = (int)(q >> 5);
        out[t] = (v < NV && j < J) ? Vw[(size_t)j * VP + v] : 0.f;
    }
}

// the workgroup's partials of one accumulator tile (acc) -> LDS -> the sum over the four waves in wave order; calls f(row, column, value)
template <typename F>
__device__ __forceinline__ void combine_tile(const f32x16 &acc, float *red, int tid, F f) {
    const int wave = tid >> 6, lane = tid & 63;
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 16; ++i) red[wave * 1024 + i * 64 + lane] = acc[i];
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int e = tid + 256 * q, i = e >> 6, ln = e & 63;
        const float s = ((red[e] + red[1024 + e]) + red[2048 + e]) + red[3072 + e];
        f(acc_row(i, ln >> 5), ln & 31, s);
    }
}

// u = scale * dL/dvert in the accumulator layout (row = hypothesis r0 + acc_row(i, half), column = vertex v); zero past R and NV
__device__ __forceinline__ void load_u(float (&u)[3][16], const float *__restrict__ g_verts, int r0, int R, int v, int NV, int half, float scale) {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int r = r0 + acc_row(i, half);
        const bool ok = v < NV && r < R;
        const float *g = g_verts + ((size_t)(ok ? r : 0) * NV + (ok ? v : 0)) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) u[c][i] = ok ? scale * g[c] : 0.f;
    }
}

// kernel G: [g_posemap | g_betas] of 32 hypotheses; NT 32-column tiles of coefficients
template <int NT>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1)))
void lbs_skin_bwd_coef_kernel(const float *__restrict__ ws, const float *__restrict__ Vw, const float *__restrict__ pdt,
                              const float *__restrict__ g_verts, float *__restrict__ g_pm, float *__restrict__ g_bt, int R, int J, int nb, int NV,
                              int VP, float scale) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int JK = (J + 1) / 2, JP = 2 * JK;
    float *Ar = sm;                                       // [9 rotation entries][JP joints][32 hypotheses]
    float *P = sm + 9 * JP * 32;                          // per wave [96 k = 3 vertex + coordinate][33]
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, vl = lane & 31, half = lane >> 5;
    const int r0 = blockIdx.x * 32;
    const int NP = 9 * (J - 1), NC = NP + nb, NCP = 32 * NT, stride = sbw_stride(J, nb), oa = NP + nb;
    for (int i = tid; i < 9 * JP * 32; i += 256) {
        const int h = i & 31, q = i >> 5, j = q % JP, e = q / JP;
        const int r = r0 + h < R ? r0 + h : R - 1;
        Ar[i] = j < J ? ws[(size_t)r * stride + oa + j * 12 + e] : 0.f;
    }
    __syncthreads();
    float *Pw = P + wave * 96 * 33;
    const int VTL = (NV + 31) / 32;
    f32x16 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[t][i] = 0.f;
    for (int vt = wave; vt < VTL; vt += 4) {
        const int v = vt * 32 + vl;                       // < VP (VP: a multiple of 32, >= NV)
        float u[3][16];
        load_u(u, g_verts, r0, R, v, NV, half, scale);
        // g_x = T[:, :3]^T u, T's rotation rows recomputed three entries at a time: T_e[h][v] = sum_j A_e[h][j] W[j][v]
        f32x16 gx[3];
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int i = 0; i < 16; ++i) gx[c][i] = 0.f;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            f32x16 T[3];
#pragma unroll
            for (int q = 0; q < 3; ++q)
#pragma unroll
                for (int i = 0; i < 16; ++i) T[q][i] = 0.f;
#pragma unroll 4
            for (int s = 0; s < JK; ++s) {
                const int j = 2 * s + half;
                const float b = j < J ? Vw[(size_t)j * VP + v] : 0.f;
#pragma unroll
                for (int q = 0; q < 3; ++q) MFMA32(Ar[((3 * a + q) * JP + j) * 32 + vl], b, T[q]);
            }
#pragma unroll
            for (int q = 0; q < 3; ++q)
#pragma unroll
                for (int i = 0; i < 16; ++i) gx[q][i] = fmaf(T[q][i], u[a][i], gx[q][i]);
        }
        // g_x -> the wave's LDS image in A-operand order (k = 3 vertex + coordinate, row = hypothesis)
        wave_sync();
#pragma unroll
        for (int i = 0; i < 16; ++i)
#pragma unroll
            for (int c = 0; c < 3; ++c) Pw[(3 * vl + c) * 33 + acc_row(i, half)] = gx[c][i];
        wave_sync();
        const float *B = pdt + (size_t)vt * 96 * NCP + vl;
#pragma unroll 4
        for (int s = 0; s < 48; ++s) {
            const int k = 2 * s + half;
            const float a = Pw[k * 33 + vl];
            const float *b = B + (size_t)k * NCP;
#pragma unroll
            for (int t = 0; t < NT; ++t) MFMA32(a, b[32 * t], acc[t]);
        }
    }
#pragma unroll
    for (int t = 0; t < NT; ++t)
        combine_tile(acc[t], P, tid, [&](int h, int cl, float s) {
            const int col = 32 * t + cl;
            if (r0 + h < R && col < NC) {
                if (col < NP) g_pm[(size_t)(r0 + h) * NP + col] = s;
                else g_bt[(size_t)(r0 + h) * nb + col - NP] = s;
            }
        });
}

// kernel A: g_transforms [J][12] of 32 hypotheses; accumulator a * 4 + b holds sum_v w_vj u_a h_b (b = 3: the homogeneous 1)
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1)))
void lbs_skin_bwd_tf_kernel(const float *__restrict__ ws, const float *__restrict__ Vt, const float *__restrict__ Vsd, const float *__restrict__ Vpd,
                            const float *__restrict__ wt, const float *__restrict__ g_verts, float *__restrict__ g_tf, int R, int J, int nb, int NV,
                            int VP, float scale) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int NP = 9 * (J - 1), NC = NP + nb, KK = (NC + 1) / 2, stride = sbw_stride(J, nb);
    float *PM = sm;                                       // [2 KK coefficients][32 hypotheses]: pose map | betas | 0
    float *Q = sm + 2 * KK * 32;                          // per wave [6 planes: u_0..2, x_0..2][32 vertices][33]
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, vl = lane & 31, half = lane >> 5;
    const int r0 = blockIdx.x * 32;
    for (int i = tid; i < 2 * KK * 32; i += 256) {
        const int h = i & 31, k = i >> 5;
        const int r = r0 + h < R ? r0 + h : R - 1;
        PM[i] = k < NC ? ws[(size_t)r * stride + k] : 0.f;
    }
    __syncthreads();
    float *Qw = Q + wave * 6 * 32 * 33;
    const int VTL = (NV + 31) / 32;
    f32x16 acc[12];
#pragma unroll
    for (int t = 0; t < 12; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[t][i] = 0.f;
    for (int vt = wave; vt < VTL; vt += 4) {
        const int v = vt * 32 + vl;
        // the forward's blend product: X_c[h][v] = vt_c[v] + sum_k PM[h][k] [PD | SD]_c[k][v]
        f32x16 X[3];
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int i = 0; i < 16; ++i) X[c][i] = 0.f;
#pragma unroll 4
        for (int s = 0; s < KK; ++s) {
            const int k = 2 * s + half;
            const float a = PM[k * 32 + vl];
            const float *src = k < NP ? Vpd + (size_t)k * 3 * VP : Vsd + (size_t)(k < NC ? k - NP : 0) * 3 * VP;
#pragma unroll
            for (int c = 0; c < 3; ++c) MFMA32(a, k < NC ? src[(size_t)c * VP + v] : 0.f, X[c]);
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float t0 = Vt[(size_t)c * VP + v];
#pragma unroll
            for (int i = 0; i < 16; ++i) X[c][i] += t0;
        }
        float u[3][16];
        load_u(u, g_verts, r0, R, v, NV, half, scale);
        wave_sync();
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int h = acc_row(i, half);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                Qw[(c * 32 + vl) * 33 + h] = u[c][i];
                Qw[((3 + c) * 32 + vl) * 33 + h] = X[c][i];
            }
        }
        wave_sync();
        const float *B = wt + (size_t)vt * 32 * 32 + vl;
#pragma unroll 4
        for (int s = 0; s < 16; ++s) {
            const int k = 2 * s + half;                   // vertex vt * 32 + k
            const float b = B[k * 32];
            float ua[3], xb[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) { ua[c] = Qw[(c * 32 + k) * 33 + vl]; xb[c] = Qw[((3 + c) * 32 + k) * 33 + vl]; }
#pragma unroll
            for (int a = 0; a < 3; ++a) {
#pragma unroll
                for (int bb = 0; bb < 3; ++bb) MFMA32(ua[a] * xb[bb], b, acc[a * 4 + bb]);
                MFMA32(ua[a], b, acc[a * 4 + 3]);
            }
        }
    }
#pragma unroll
    for (int t = 0; t < 12; ++t) {
        const int a = t >> 2, bb = t & 3, e = bb < 3 ? 3 * a + bb : 9 + a;     // the workspace's transform layout: rotation row-major, then a_j
        combine_tile(acc[t], Q, tid, [&](int h, int j, float s) {
            if (r0 + h < R && j < J) g_tf[((size_t)(r0 + h) * J + j) * 12 + e] = s;
        });
    }
}

template <int NT>
static void launch_coef(dim3 grid, size_t lds, hipStream_t st, const float *ws, const float *Vw, const float *pdt, const float *g_verts, float *g_pm,
                        float *g_bt, int R, int J, int nb, int NV, int VP, float scale) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(lbs_skin_bwd_coef_kernel<NT>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(lbs_skin_bwd_coef_kernel<NT>, grid, dim3(256), lds, st, ws, Vw, pdt, g_verts, g_pm, g_bt, R, J, nb, NV, VP, scale);
}

}}  // namespace mhe::body

using namespace mhe;

extern "C" size_t mhe_lbs_bwd_tables_floats(int J, int nb, int VP) {
    if (J <= 1 || J > 32 || nb <= 0 || nb > 64 || VP <= 0 || VP % 32) return 0;
    return body::sbw_tables_floats(J, nb, VP);
}

extern "C" int mhe_lbs_bwd_tables_f32(const float *v_shapedirs, const float *v_posedirs, const float *v_weights, float *tables, int J, int nb, int NV,
                                      int VP, void *stream) {
    MHE_REQUIRE(v_shapedirs && v_posedirs && v_weights && tables, "mhe_lbs_bwd_tables_f32: null pointer");
    MHE_REQUIRE(J > 1 && J <= 32 && nb > 0 && nb <= 64 && NV > 0 && VP >= NV && VP % 32 == 0,
                "mhe_lbs_bwd_tables_f32: J=%d nb=%d NV=%d VP=%d (1 < J <= 32, 0 < nb <= 64, VP >= NV a multiple of 32)", J, nb, NV, VP);
    MHE_REQUIRE(on_device(v_shapedirs) && on_device(v_posedirs) && on_device(v_weights) && on_device(tables),
                "mhe_lbs_bwd_tables_f32: every buffer must be device memory");
    const long n = (long)body::sbw_tables_floats(J, nb, VP);
    hipLaunchKernelGGL(body::lbs_bwd_tables_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, v_shapedirs, v_posedirs,
                       v_weights, tables, J, nb, NV, VP);
    return check_launch("lbs_bwd_tables_kernel");
}

extern "C" int mhe_lbs_skin_bwd_f32(const float *workspace, const float *v_template, const float *v_shapedirs, const float *v_posedirs,
                                    const float *v_weights, const float *tables, const float *g_verts, float *g_transforms, float *g_posemap,
                                    float *g_betas, int R, int J, int nb, int NV, int VP, float scale, void *stream) {
    MHE_REQUIRE(workspace && v_template && v_shapedirs && v_posedirs && v_weights && tables && g_verts && g_transforms && g_posemap && g_betas,
                "mhe_lbs_skin_bwd_f32: null pointer");
    MHE_REQUIRE(R > 0 && J > 1 && J <= 32 && nb > 0 && nb <= 64 && NV > 0 && VP >= NV && VP % 32 == 0,
                "mhe_lbs_skin_bwd_f32: R=%d J=%d nb=%d NV=%d VP=%d (1 < J <= 32, 0 < nb <= 64, VP >= NV a multiple of 32)", R, J, nb, NV, VP);
    MHE_REQUIRE(on_device(workspace) && on_device(tables) && on_device(g_verts) && on_device(g_transforms) && on_device(g_posemap) &&
                    on_device(g_betas), "mhe_lbs_skin_bwd_f32: every buffer must be device memory");
    const dim3 grid((unsigned)((R + 31) / 32));
    const hipStream_t st = (hipStream_t)stream;
    const int NT = body::sbw_nt(J, nb);
    const float *pdt = tables, *wt = tables + (size_t)VP * 3 * 32 * NT;
    const size_t lg = body::sbw_lds_g(J), la = body::sbw_lds_a(J, nb);
    switch (NT) {
#define MHE_COEF_CASE(n) case n: body::launch_coef<n>(grid, lg, st, workspace, v_weights, pdt, g_verts, g_posemap, g_betas, R, J, nb, NV, VP, scale); break;
        MHE_COEF_CASE(1) MHE_COEF_CASE(2) MHE_COEF_CASE(3) MHE_COEF_CASE(4) MHE_COEF_CASE(5) MHE_COEF_CASE(6)
        MHE_COEF_CASE(7) MHE_COEF_CASE(8) MHE_COEF_CASE(9) MHE_COEF_CASE(10) MHE_COEF_CASE(11)
#undef MHE_COEF_CASE
        default: MHE_REQUIRE(false, "mhe_lbs_skin_bwd_f32: %d coefficient tiles", NT);
    }
    int rc = check_launch("lbs_skin_bwd_coef_kernel");
    if (rc) return rc;
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(body::lbs_skin_bwd_tf_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)la);
    hipLaunchKernelGGL(body::lbs_skin_bwd_tf_kernel, grid, dim3(256), la, st, workspace, v_template, v_shapedirs, v_posedirs, wt, g_verts, g_transforms,
                       R, J, nb, NV, VP, scale);
    return check_launch("lbs_skin_bwd_tf_kernel");
}
