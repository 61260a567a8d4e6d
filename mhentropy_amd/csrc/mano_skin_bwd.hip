// Reverse of the hand's full-mesh skinning (mano_skin_mfma_kernel, csrc/mano_skin.hip; the arithmetic of hand/manopth/manolayer.py:181-246,
// :262-273 and hand/network.py:480) on the matrix cores in EXACT f32: v_mfma_f32_32x32x2_f32, a k-ordered fmaf chain per output.  It is the scheme
// of csrc/lbs_skin_bwd.hip at MANO's compile-time sizes (16 joints, 10 betas, 135 pose-map entries, 778 vertices padded to 832) on the hand's
// workspace row (mano_layout.h).  With x_v = vt_v + SD_v beta + PD_v pm, h_v = [x_v; 1], T_v = sum_j w_vj G_j, vp_v = T_v h_v and
//   mesh_v = (vp_v - centre) 1000 [mm_mode],  verts_v = (mesh_v - root) / bone [normalised],
// an incoming g_v = dL/dverts_v gives u_v = s g_v with the ROW's scale s = 1000 (mm_mode) or 1000 / bone, and
//   g_G_j = sum_v w_vj u_v h_v^T                                        (kernel A: mano_skin_bwd_tf_kernel, the forward's blend product X recomputed)
//   g_x_v = T_v[:, :3]^T u_v;  [g_pm | g_beta] = sum_v [PD_v | SD_v]^T g_x_v      (kernel G: mano_skin_bwd_coef_kernel, T's rotation part recomputed)
//   S = sum_v u_v,  D = sum_v u_v . vp_v = sum_j <G_j, g_G_j>  (vp is linear in the transforms)              (kernel A's epilogue)
//   g_centre = -S;  normalised mode: g_root = -S / 1000,  g_bone = -(D - S . (centre + root / 1000)) / bone = -(1 / bone) sum_v g_v . verts_v
// S costs nothing: column 16 of the weight table is 1 for every vertex, so the homogeneous accumulators carry it next to the 16 joints.
// The row scale is applied where g_verts is loaded: there is no sweep over g_verts before these two kernels.
// Vertex = k of the MFMA, hypothesis = row (32 per workgroup, A operands from LDS), coefficient / joint = column (B operands: coefficient-
// fastest tables that mano_bwd_tables_kernel makes from the packed blob's vertex section on every call, into the caller's workspace).  Per
// 32-vertex tile a wave recomputes what the forward had in the accumulator layout (vertex = lane), forms g_x / u / x lane-locally and moves them
// through a wave-private LDS image into A-operand layout.  Wave w visits tiles w, w + 4, ...; the four waves' partials are summed in wave order.
// Vertices 778..831 and rows past R are loaded as zeros (never read from g_verts).  No atomics: two calls give the same bits.
// Output: one adjoint row per hypothesis with the workspace row's own layout (WS_PM | WS_BT | WS_GR | WS_NRM = g_centre, g_root, g_bone).
// The pose chain's reverse is mano_verts_bwd_kernel (mano_bwd.hip).  First version, not tuned.
#include "common.h"
#include "mano_layout.h"

namespace mhe { namespace mano {

typedef __attribute__((ext_vector_type(16))) float f32x16;
#define MFMA32(a, b, c) c = __builtin_amdgcn_mfma_f32_32x32x2f32((a), (b), (c), 0, 0, 0)

constexpr int NJ = 16, NPM = 135, NC = 145;               // joints; pose-map entries; coefficients = pose map | betas (WS_PM, WS_BT: contiguous)
constexpr int NCT = 5, NCP = 32 * NCT;                    // coefficient columns of kernel G in whole 32-column tiles
constexpr int KK = (NC + 1) / 2;                          // k-steps of kernel A's blend product
constexpr int VTL = (NV + 31) / 32;                       // 25 vertex tiles hold vertices
constexpr int ONES_COL = 16;                              // column of WT that is 1 for every vertex
constexpr size_t BT_PD = 0;                               // PDT [VP][3][NCP]: row = (vertex, coordinate), column = coefficient
constexpr size_t BT_W = (size_t)VP * 3 * NCP;             // WT [VP][32]: column = joint (16), then ONES_COL, then zeros
constexpr size_t BT_FLOATS = BT_W + (size_t)VP * 32;
constexpr size_t LDS_G = ((size_t)9 * NJ * 32 + 4 * 96 * 33 + 32) * 4;
constexpr size_t LDS_A = ((size_t)2 * KK * 32 + 4 * 6 * 32 * 33 + 32) * 4;

__device__ __forceinline__ int acc_row(int i, int half) { return (i & 3) + 8 * (i >> 2) + 4 * half; }

__global__ __launch_bounds__(256) void mano_bwd_tables_kernel(const float *__restrict__ tables, float *__restrict__ out) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t < (int)BT_W) {
        const int k = t % NCP, rc = t / NCP, c = rc % 3, v = rc / 3;
        float x = 0.f;
        if (v < NV && k < NC) x = k < NPM ? tables[V_PD + (k * 3 + c) * VP + v] : tables[V_SD + ((k - NPM) * 3 + c) * VP + v];
        out[t] = x;
    } else if (t < (int)BT_FLOATS) {
        const int q = t - (int)BT_W, j = q & 31, v = q >> 5;
        out[t] = v < NV ? (j < NJ ? tables[V_W + j * VP + v] : (j == ONES_COL ? 1.f : 0.f)) : 0.f;
    }
}

// the workgroup's partials of one accumulator tile (acc) -> LDS -> the sum over the four waves in wave order; calls f(q, row, column, value),
// q = 0..3: the thread's q-th element, the same (row, column) for every tile
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
        f(q, acc_row(i, ln >> 5), ln & 31, s);
    }
}

// the output scale of the workgroup's 32 rows: 1000 (mm_mode) or 1000 / bone
__device__ __forceinline__ void load_scales(float *scl, const float *__restrict__ ws, int r0, int R, int mm_mode, int tid) {
    if (tid < 32) {
        const int r = r0 + tid < R ? r0 + tid : R - 1;
        scl[tid] = mm_mode ? 1000.f : 1000.f / ws[(size_t)r * WS_STRIDE + WS_NRM + 6];
    }
}

// u = scale[row] * dL/dverts in the accumulator layout (row = hypothesis r0 + acc_row(i, half), column = vertex v); zero past R and NV
__device__ __forceinline__ void load_u(float (&u)[3][16], const float *__restrict__ g_verts, const float *scl, int r0, int R, int v, int half) {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int h = acc_row(i, half), r = r0 + h;
        const bool ok = v < NV && r < R;
        const float *g = g_verts + ((size_t)(ok ? r : 0) * NV + (ok ? v : 0)) * 3;
        const float s = scl[h];
#pragma unroll
        for (int c = 0; c < 3; ++c) u[c][i] = ok ? s * g[c] : 0.f;
    }
}

// kernel G: [g_pm | g_beta] of 32 hypotheses
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1)))
void mano_skin_bwd_coef_kernel(const float *__restrict__ ws, const float *__restrict__ tables, const float *__restrict__ pdt,
                               const float *__restrict__ g_verts, float *__restrict__ adj, int R, int mm_mode) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float *Ar = sm;                                       // [9 rotation entries][16 joints][32 hypotheses]
    float *P = sm + 9 * NJ * 32;                          // per wave [96 k = 3 vertex + coordinate][33]
    float *scl = P + 4 * 96 * 33;                         // [32]
    const float *Vw = tables + V_W;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, vl = lane & 31, half = lane >> 5;
    const int r0 = blockIdx.x * 32;
    for (int i = tid; i < 9 * NJ * 32; i += 256) {
        const int h = i & 31, q = i >> 5, j = q % NJ, e = q / NJ;
        const int r = r0 + h < R ? r0 + h : R - 1;
        Ar[i] = ws[(size_t)r * WS_STRIDE + WS_GR + j * 12 + e];
    }
    load_scales(scl, ws, r0, R, mm_mode, tid);
    __syncthreads();
    float *Pw = P + wave * 96 * 33;
    f32x16 acc[NCT];
#pragma unroll
    for (int t = 0; t < NCT; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[t][i] = 0.f;
    for (int vt = wave; vt < VTL; vt += 4) {
        const int v = vt * 32 + vl;                       // < VP
        float u[3][16];
        load_u(u, g_verts, scl, r0, R, v, half);
        // g_x = T[:, :3]^T u, T's rotation rows recomputed three entries at a time: T_e[h][v] = sum_j G_e[h][j] W[j][v]
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
            for (int s = 0; s < NJ / 2; ++s) {
                const int j = 2 * s + half;
                const float b = Vw[j * VP + v];
#pragma unroll
                for (int q = 0; q < 3; ++q) MFMA32(Ar[((3 * a + q) * NJ + j) * 32 + vl], b, T[q]);
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
            for (int t = 0; t < NCT; ++t) MFMA32(a, b[32 * t], acc[t]);
        }
    }
#pragma unroll
    for (int t = 0; t < NCT; ++t)
        combine_tile(acc[t], P, tid, [&](int, int h, int cl, float s) {
            const int col = 32 * t + cl;                  // WS_PM | WS_BT: the adjoint row's first 145 floats
            if (r0 + h < R && col < NC) adj[(size_t)(r0 + h) * WS_STRIDE + col] = s;
        });
}

// kernel A: g_G [16][12] of 32 hypotheses and the normalisation adjoints; accumulator a * 4 + b holds sum_v w_vj u_a h_b (b = 3: the homogeneous 1)
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1)))
void mano_skin_bwd_tf_kernel(const float *__restrict__ ws, const float *__restrict__ tables, const float *__restrict__ wt,
                             const float *__restrict__ g_verts, float *__restrict__ adj, int R, int mm_mode) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float *PM = sm;                                       // [2 KK coefficients][32 hypotheses]: pose map | betas | 0; after the tiles: S [3][32], D [32]
    float *Q = sm + 2 * KK * 32;                          // per wave [6 planes: u_0..2, x_0..2][32 vertices][33]
    float *scl = Q + 4 * 6 * 32 * 33;                     // [32]
    const float *Vt = tables + V_T, *Vsd = tables + V_SD, *Vpd = tables + V_PD;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, vl = lane & 31, half = lane >> 5;
    const int r0 = blockIdx.x * 32;
    for (int i = tid; i < 2 * KK * 32; i += 256) {
        const int h = i & 31, k = i >> 5;
        const int r = r0 + h < R ? r0 + h : R - 1;
        PM[i] = k < NC ? ws[(size_t)r * WS_STRIDE + k] : 0.f;
    }
    load_scales(scl, ws, r0, R, mm_mode, tid);
    __syncthreads();
    float *Qw = Q + wave * 6 * 32 * 33;
    // the blend loop's trip count, hidden from the optimiser: with the constant in sight it schedules the whole 73-step loop as one block and
    // spills 436 bytes per lane next to the twelve accumulator tiles (216 registers and no scratch this way)
    int ksteps = KK;
    asm volatile("" : "+s"(ksteps));
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
        for (int s = 0; s < ksteps; ++s) {
            const int k = 2 * s + half;
            const float a = PM[k * 32 + vl];
            const float *src = k < NPM ? Vpd + k * 3 * VP : Vsd + (k < NC ? k - NPM : 0) * 3 * VP;
#pragma unroll
            for (int c = 0; c < 3; ++c) MFMA32(a, k < NC ? src[c * VP + v] : 0.f, X[c]);
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float t0 = Vt[c * VP + v];
#pragma unroll
            for (int i = 0; i < 16; ++i) X[c][i] += t0;
        }
        float u[3][16];
        load_u(u, g_verts, scl, r0, R, v, half);
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
    // g_G in the workspace's transform layout (rotation row-major, then the translation); D = <G, g_G> per (row, joint) on the way
    float dpart[4] = {0.f, 0.f, 0.f, 0.f};
    float *Ss = PM, *Ds = PM + 96;                        // (PM is free: combine_tile's first barrier is past every wave's tiles)
#pragma unroll
    for (int t = 0; t < 12; ++t) {
        const int a = t >> 2, bb = t & 3, e = bb < 3 ? 3 * a + bb : 9 + a;
        combine_tile(acc[t], Q, tid, [&](int q, int h, int j, float s) {
            if (j < NJ) {
                const int r = r0 + h < R ? r0 + h : R - 1;
                dpart[q] = fmaf(s, ws[(size_t)r * WS_STRIDE + WS_GR + j * 12 + e], dpart[q]);
                if (r0 + h < R) adj[(size_t)(r0 + h) * WS_STRIDE + WS_GR + j * 12 + e] = s;
            } else if (bb == 3 && j == ONES_COL) Ss[a * 32 + h] = s;
        });
    }
    // the 16 joints of a row sit on 16 consecutive lanes (columns 16..31 hold zeros and reduce among themselves)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        float d = dpart[q];
#pragma unroll
        for (int of = 8; of > 0; of >>= 1) d += __shfl_xor(d, of, 64);
        const int el = tid + 256 * q, i = el >> 6, ln = el & 63;
        if ((ln & 31) == 0) Ds[acc_row(i, ln >> 5)] = d;
    }
    __syncthreads();
    if (tid < 32 && r0 + tid < R) {
        const float *w = ws + (size_t)(r0 + tid) * WS_STRIDE + WS_NRM;      // centre (m), root (mm, centred), bone (mm)
        float *o = adj + (size_t)(r0 + tid) * WS_STRIDE + WS_NRM;
        const float S0 = Ss[tid], S1 = Ss[32 + tid], S2 = Ss[64 + tid];
        o[0] = -S0; o[1] = -S1; o[2] = -S2;
        if (mm_mode) {
            o[3] = 0.f; o[4] = 0.f; o[5] = 0.f; o[6] = 0.f;
        } else {
            o[3] = -S0 / 1000.f; o[4] = -S1 / 1000.f; o[5] = -S2 / 1000.f;
            const float off = S0 * (w[0] + w[3] / 1000.f) + S1 * (w[1] + w[4] / 1000.f) + S2 * (w[2] + w[5] / 1000.f);
            o[6] = -(Ds[tid] - off) / w[6];
        }
    }
}

}}  // namespace mhe::mano

using namespace mhe;

size_t mhe_mano_skin_bwd_table_floats() { return mano::BT_FLOATS; }

// ws_rows: the forward's workspace rows (mano_pose_kernel); bt: mhe_mano_skin_bwd_table_floats() floats, written here; adj: [R][WS_STRIDE]
int mhe_mano_skin_bwd(const float *ws_rows, const float *tables, float *bt, const float *g_verts, float *adj, int R, int mm_mode,
                      hipStream_t stream) {
    hipLaunchKernelGGL(mano::mano_bwd_tables_kernel, dim3((unsigned)((mano::BT_FLOATS + 255) / 256)), dim3(256), 0, stream, tables, bt);
    if (int rc = check_launch("mano_bwd_tables_kernel")) return rc;
    const dim3 grid((unsigned)((R + 31) / 32));
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(mano::mano_skin_bwd_coef_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)mano::LDS_G);
    hipLaunchKernelGGL(mano::mano_skin_bwd_coef_kernel, grid, dim3(256), mano::LDS_G, stream, ws_rows, tables, bt + mano::BT_PD, g_verts, adj, R,
                       mm_mode);
    if (int rc = check_launch("mano_skin_bwd_coef_kernel")) return rc;
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(mano::mano_skin_bwd_tf_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)mano::LDS_A);
    hipLaunchKernelGGL(mano::mano_skin_bwd_tf_kernel, grid, dim3(256), mano::LDS_A, stream, ws_rows, tables, bt + mano::BT_W, g_verts, adj, R,
                       mm_mode);
    return check_launch("mano_skin_bwd_tf_kernel");
}
