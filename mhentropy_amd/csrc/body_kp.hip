// Body keypoints, the parts around the skinning kernels (lbs_skin.hip, body.hip):
//   reverse of keypoints = regressor x vertices:  g_verts (R,NV,3) (+)= regressor^T g_keypoints  (feeds mhe_lbs_skin_bwd_f32 unchanged),
//   the 2D keypoint likelihood of the K hypotheses and its reverse: orthographic projection proj = s xy + t (reference hand/ManoLayer.py:150-165,
//   batch_orth_proj with inv_norm=False) under the visibility-masked Laplace density of hand/network.py:233-258 (b_type 'const'):
//       log_p = sum over NK x 2 of [vis == 1] (-(relu(|uv - proj| - 1e-4) + 1e-4) / b - log(2 b)).
// Sums over the <= 64 keypoints are wave butterflies, sums over the K hypotheses of a shared camera run in a fixed order: no atomics.
#include "common.h"

namespace mhe { namespace body {

constexpr int KPB_HB = 8;

// one thread per vertex, KPB_HB hypotheses per workgroup (their keypoint gradients in LDS, every regressor element read once per workgroup)
__global__ __launch_bounds__(256) void lbs_keypoints_bwd_kernel(const float *__restrict__ reg, const float *__restrict__ g_kp, float *g_verts, int R, int NK,
                                                                int NV, int accumulate) {
    __shared__ float sG[KPB_HB][64 * 3];
    const int v = blockIdx.x * 256 + threadIdx.x, r0 = blockIdx.y * KPB_HB;
    for (int i = threadIdx.x; i < KPB_HB * NK * 3; i += 256) {
        const int h = i / (NK * 3), e = i - h * NK * 3;
        sG[h][e] = r0 + h < R ? g_kp[(size_t)(r0 + h) * NK * 3 + e] : 0.f;
    }
    __syncthreads();
    if (v >= NV) return;
    float acc[KPB_HB][3];
#pragma unroll
    for (int h = 0; h < KPB_HB; ++h) acc[h][0] = acc[h][1] = acc[h][2] = 0.f;
    for (int k = 0; k < NK; ++k) {
        const float w = reg[(size_t)k * NV + v];
#pragma unroll
        for (int h = 0; h < KPB_HB; ++h) {
            acc[h][0] = fmaf(w, sG[h][3 * k], acc[h][0]); acc[h][1] = fmaf(w, sG[h][3 * k + 1], acc[h][1]); acc[h][2] = fmaf(w, sG[h][3 * k + 2], acc[h][2]);
        }
    }
#pragma unroll
    for (int h = 0; h < KPB_HB; ++h) {
        if (r0 + h < R) {
            float *o = g_verts + ((size_t)(r0 + h) * NV + v) * 3;
#pragma unroll
            for (int c = 0; c < 3; ++c) o[c] = accumulate ? o[c] + acc[h][c] : acc[h][c];
        }
    }
}

constexpr float KP_EPS = 1e-4f;          // network.py:233-258: the dead zone of the Laplace term

// one wavefront per (image, hypothesis) row, lane = keypoint
__global__ __launch_bounds__(256) void kp_log_prob_kernel(const float *__restrict__ kp, const float *__restrict__ cam, const float *__restrict__ uv,
                                                          const float *__restrict__ vis, float *__restrict__ log_p, int B, int K, int NK, int cam_per_hyp,
                                                          float b, float log2b) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= (long)B * K) return;
    const int img = (int)(row / K);
    const float *cm = cam + (cam_per_hyp ? row : img) * 3;
    const float s = cm[0], tx = cm[1], ty = cm[2];
    float t = 0.f;
    if (lane < NK && vis[(size_t)img * NK + lane] == 1.f) {
        const float *p = kp + ((size_t)row * NK + lane) * 3, *y = uv + ((size_t)img * NK + lane) * 2;
        const float du = fabsf(y[0] - (s * p[0] + tx)), dv = fabsf(y[1] - (s * p[1] + ty));
        t = (-(fmaxf(du - KP_EPS, 0.f) + KP_EPS) / b - log2b) + (-(fmaxf(dv - KP_EPS, 0.f) + KP_EPS) / b - log2b);
    }
    t = wave_sum(t);
    if (lane == 0) log_p[row] = t;
}

// one workgroup per image; wave w takes hypotheses w, w + 4, ... in order; a shared camera's gradient: each wave's running sum over its
// hypotheses, then ((w0 + w1) + w2) + w3
__global__ __launch_bounds__(256) void kp_log_prob_bwd_kernel(const float *__restrict__ kp, const float *__restrict__ cam, const float *__restrict__ uv,
                                                              const float *__restrict__ vis, const float *__restrict__ g, float *__restrict__ g_kp,
                                                              float *__restrict__ g_cam, int K, int NK, int cam_per_hyp, float b) {
    __shared__ float sC[4][3];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, img = blockIdx.x;
    const bool on = lane < NK && vis[(size_t)img * NK + (lane < NK ? lane : 0)] == 1.f;
    float yu = 0.f, yv = 0.f;
    if (on) { yu = uv[((size_t)img * NK + lane) * 2]; yv = uv[((size_t)img * NK + lane) * 2 + 1]; }
    float a0 = 0.f, a1 = 0.f, a2 = 0.f;
    for (int k = wave; k < K; k += 4) {
        const size_t row = (size_t)img * K + k;
        const float *cm = cam + (cam_per_hyp ? row : (size_t)img) * 3;
        const float s = cm[0], tx = cm[1], ty = cm[2], gr = g[row] / b;
        float gu = 0.f, gv = 0.f, x = 0.f, y = 0.f;
        if (on) {
            const float *p = kp + (row * NK + lane) * 3;
            x = p[0]; y = p[1];
            const float du = yu - (s * x + tx), dv = yv - (s * y + ty);
            // d log_p / d proj = sign(uv - proj) / b outside the dead zone, 0 inside it
            gu = fabsf(du) - KP_EPS > 0.f ? (du > 0.f ? gr : -gr) : 0.f;
            gv = fabsf(dv) - KP_EPS > 0.f ? (dv > 0.f ? gr : -gr) : 0.f;
        }
        if (lane < NK) {
            float *o = g_kp + (row * NK + lane) * 3;
            o[0] = s * gu; o[1] = s * gv; o[2] = 0.f;
        }
        const float gs = wave_sum(gu * x + gv * y), gx = wave_sum(gu), gy = wave_sum(gv);
        if (cam_per_hyp) {
            if (lane == 0) { g_cam[row * 3] = gs; g_cam[row * 3 + 1] = gx; g_cam[row * 3 + 2] = gy; }
        } else { a0 += gs; a1 += gx; a2 += gy; }
    }
    if (!cam_per_hyp) {
        if (lane == 0) { sC[wave][0] = a0; sC[wave][1] = a1; sC[wave][2] = a2; }
        __syncthreads();
        if (threadIdx.x < 3) g_cam[(size_t)img * 3 + threadIdx.x] = ((sC[0][threadIdx.x] + sC[1][threadIdx.x]) + sC[2][threadIdx.x]) + sC[3][threadIdx.x];
    }
}

}}  // namespace mhe::body

using namespace mhe;

extern "C" int mhe_lbs_keypoints_bwd_f32(const float *regressor, const float *g_keypoints, float *g_verts, int R, int NK, int NV, int accumulate,
                                         void *stream) {
    MHE_REQUIRE(NK >= 1 && NK <= 64, "mhe_lbs_keypoints_bwd_f32: NK=%d outside 1..64", NK);
    MHE_REQUIRE(regressor && g_keypoints && g_verts, "mhe_lbs_keypoints_bwd_f32: null pointer");
    MHE_REQUIRE(R > 0 && NV > 0 && (R + body::KPB_HB - 1) / body::KPB_HB <= 65535, "mhe_lbs_keypoints_bwd_f32: R=%d NV=%d (0 < R <= 524,280 rows per call)", R, NV);
    hipLaunchKernelGGL(body::lbs_keypoints_bwd_kernel, dim3((NV + 255) / 256, (R + body::KPB_HB - 1) / body::KPB_HB), dim3(256), 0, (hipStream_t)stream,
                       regressor, g_keypoints, g_verts, R, NK, NV, accumulate);
    return check_launch("lbs_keypoints_bwd_kernel");
}

extern "C" int mhe_kp_log_prob_f32(const float *keypoints, const float *cam, const float *uv, const float *vis, float *log_p, int B, int K, int NK,
                                   int cam_per_hyp, float b, void *stream) {
    MHE_REQUIRE(NK >= 1 && NK <= 64, "mhe_kp_log_prob_f32: NK=%d outside 1..64", NK);
    MHE_REQUIRE(keypoints && cam && uv && vis && log_p, "mhe_kp_log_prob_f32: null pointer");
    MHE_REQUIRE(B > 0 && K > 0 && b > 0.f, "mhe_kp_log_prob_f32: B=%d K=%d b=%g", B, K, (double)b);
    const long rows = (long)B * K;
    hipLaunchKernelGGL(body::kp_log_prob_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, keypoints, cam, uv, vis, log_p, B, K,
                       NK, cam_per_hyp, b, logf(2.f * b));
    return check_launch("kp_log_prob_kernel");
}

extern "C" int mhe_kp_log_prob_bwd_f32(const float *keypoints, const float *cam, const float *uv, const float *vis, const float *g, float *g_keypoints,
                                       float *g_cam, int B, int K, int NK, int cam_per_hyp, float b, void *stream) {
    MHE_REQUIRE(NK >= 1 && NK <= 64, "mhe_kp_log_prob_bwd_f32: NK=%d outside 1..64", NK);
    MHE_REQUIRE(keypoints && cam && uv && vis && g && g_keypoints && g_cam, "mhe_kp_log_prob_bwd_f32: null pointer");
    MHE_REQUIRE(B > 0 && K > 0 && b > 0.f, "mhe_kp_log_prob_bwd_f32: B=%d K=%d b=%g", B, K, (double)b);
    hipLaunchKernelGGL(body::kp_log_prob_bwd_kernel, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, keypoints, cam, uv, vis, g, g_keypoints, g_cam, K,
                       NK, cam_per_hyp, b);
    return check_launch("kp_log_prob_bwd_kernel");
}
