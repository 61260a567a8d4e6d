// Hand mesh evaluation (criteria.mesh_eval, ops.mesh_eval): the vertex-to-vertex error of every hypothesis' mesh against its image's ground-truth
// mesh and precision / recall / F-score of the two vertex sets at up to four distance thresholds (the FreiHAND / HO3D protocol), without the
// (N B, V, V) distance tensor of the torch route.
//   p_v = pred[r][v] (scale[b] unit),  g_v = target[b][v] (scale[b] unit),  err[r] = (1/V) sum_v |p_v - g_v|
//   d1_v = min_w |p_v - g_w|,  d2_w = min_v |p_v - g_w|,  P_t = #{v: d1_v < thr_t} / V,  R_t = #{w: d2_w < thr_t} / V,  F_t = 2 P R / (P + R)
// f32.  The minima are taken of SQUARED distances, one square root per minimum, and the DISTANCE sqrtf(min) is what is compared with thr_t, by a
// strict <, as the FreiHAND / HO3D evaluation code does (a vertex exactly thr away is not counted).  Fixed summation order, integer counts, no
// atomics: two launches give the same bits.
#include <algorithm>
#include "common.h"

namespace mhe { namespace mesh_eval {

constexpr int NT = 256;                              // threads of a workgroup: 4 waves, one per SIMD; 5 workgroups per CU at V = 778 (82 VGPRs), 8 at V <= 512 (LDS 19 KB)
constexpr int VMAX = MHE_CHAMFER_MAX_POINTS;         // 778
constexpr int KMAX = (VMAX + NT - 1) / NT;           // vertices of one thread, of either set
constexpr int VP = (VMAX + 3) / 4 * 4;               // a plane's floats: the scan reads four at a time
constexpr int TMAX = MHE_MESH_EVAL_MAX_THRESHOLDS;
constexpr int WG_TARGET = 2048;                      // workgroups asked for: 8 per CU on 256 CUs
static_assert(KMAX == 4, "the entry's switch instantiates K = 1..4");

struct Thr { int T; float v[TMAX]; };

__device__ __forceinline__ float sqdist(float ax, float ay, float az, float bx, float by, float bz) {
    const float dx = ax - bx, dy = ay - by, dz = az - bz;
    return fmaf(dz, dz, fmaf(dy, dy, dx * dx));
}

// m[k] = min over the V points of the planes (sx, sy, sz) of the squared distance to the thread's K points (ax, ay, az)[k].  Every lane reads the
// same address: a 16-byte LDS broadcast per plane serves four points for all K own points of all 64 lanes (3 reads per 28 K vector operations).
template <int K>
__device__ __forceinline__ void scan(const float *sx, const float *sy, const float *sz, int V, const float *ax, const float *ay, const float *az, float *m) {
#pragma unroll
    for (int k = 0; k < K; ++k) m[k] = __builtin_inff();
    int v = 0;
#pragma unroll 2
    for (; v + 4 <= V; v += 4) {
        const float4 X = *reinterpret_cast<const float4 *>(sx + v), Y = *reinterpret_cast<const float4 *>(sy + v), Z = *reinterpret_cast<const float4 *>(sz + v);
#pragma unroll
        for (int k = 0; k < K; ++k) {
            m[k] = fminf(m[k], sqdist(ax[k], ay[k], az[k], X.x, Y.x, Z.x));
            m[k] = fminf(m[k], sqdist(ax[k], ay[k], az[k], X.y, Y.y, Z.y));
            m[k] = fminf(m[k], sqdist(ax[k], ay[k], az[k], X.z, Y.z, Z.z));
            m[k] = fminf(m[k], sqdist(ax[k], ay[k], az[k], X.w, Y.w, Z.w));
        }
    }
    for (; v < V; ++v) {
        const float x = sx[v], y = sy[v], z = sz[v];
#pragma unroll
        for (int k = 0; k < K; ++k) m[k] = fminf(m[k], sqdist(ax[k], ay[k], az[k], x, y, z));
    }
}

__device__ __forceinline__ int wave_sum_int(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// Workgroup (b, c): image b, hypotheses n0 .. n0 + g - 1.  The image's scaled target mesh goes to LDS (x / y / z planes) once; every hypothesis is
// staged next to it the same way.  Thread tid owns vertices tid + k NT (k < K) of BOTH sets in registers: with the target planes it finds d1 of its
// predicted vertices, with the hypothesis' planes d2 of its target vertices.  Per hypothesis two barriers: planes staged | partial sums in LDS.
// The waves' partial sums are added in wave order, the counts are integers.
template <int K>
__global__ __launch_bounds__(NT) void mesh_eval_kernel(const float *__restrict__ pred, const float *__restrict__ target, const float *__restrict__ scale,
                                                       float *__restrict__ err, float *__restrict__ prf, int N, int B, int V, int G, int chunks, float unit,
                                                       Thr thr) {
    __shared__ __attribute__((aligned(16))) float tg[3][VP];
    __shared__ __attribute__((aligned(16))) float hy[3][VP];
    __shared__ float red_e[NT / 64];
    __shared__ int red_c[NT / 64][TMAX];          // (recall count << 16) | precision count, each at most 778
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.x / chunks, n0 = (blockIdx.x % chunks) * G;
    const int g = min(G, N - n0);
    const float su = scale[b] * unit;
    const size_t R = (size_t)N * B;

    float gx[K], gy[K], gz[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int v = k * NT + tid;
        gx[k] = gy[k] = gz[k] = 0.f;
        if (v < V) {
            const float *t = target + ((size_t)b * V + v) * 3;
            gx[k] = t[0] * su; gy[k] = t[1] * su; gz[k] = t[2] * su;
            tg[0][v] = gx[k]; tg[1][v] = gy[k]; tg[2][v] = gz[k];
        }
    }
    for (int n = 0; n < g; ++n) {
        const size_t r = (size_t)(n0 + n) * B + b;
        float px[K], py[K], pz[K];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int v = k * NT + tid;
            px[k] = py[k] = pz[k] = 0.f;
            if (v < V) {
                const float *p = pred + (r * V + v) * 3;
                px[k] = p[0] * su; py[k] = p[1] * su; pz[k] = p[2] * su;
                hy[0][v] = px[k]; hy[1][v] = py[k]; hy[2][v] = pz[k];
            }
        }
        __syncthreads();                           // the hypothesis is staged (first pass: the target as well); red_* of the last one are read
        float m1[K], m2[K];
        scan<K>(tg[0], tg[1], tg[2], V, px, py, pz, m1);
        scan<K>(hy[0], hy[1], hy[2], V, gx, gy, gz, m2);
        float e = 0.f;
        int c[TMAX] = {0, 0, 0, 0};
#pragma unroll
        for (int k = 0; k < K; ++k)
            if (k * NT + tid < V) {
                e += sqrtf(sqdist(px[k], py[k], pz[k], gx[k], gy[k], gz[k]));
                const float d1 = sqrtf(m1[k]), d2 = sqrtf(m2[k]);
#pragma unroll
                for (int t = 0; t < TMAX; ++t)
                    if (t < thr.T) c[t] += (d1 < thr.v[t] ? 1 : 0) + (d2 < thr.v[t] ? 1 << 16 : 0);
            }
        e = wave_sum(e);
#pragma unroll
        for (int t = 0; t < TMAX; ++t)
            if (t < thr.T) c[t] = wave_sum_int(c[t]);
        if (lane == 0) {
            red_e[wave] = e;
#pragma unroll
            for (int t = 0; t < TMAX; ++t) red_c[wave][t] = c[t];
        }
        __syncthreads();                           // the partial sums are written; nobody reads hy[] any more
        if (tid < thr.T) {
            const int cs = red_c[0][tid] + red_c[1][tid] + red_c[2][tid] + red_c[3][tid], cp = cs & 0xffff, cr = cs >> 16;
            float *o = prf + (size_t)tid * R + r;
            const size_t plane = (size_t)thr.T * R;
            o[0] = (float)cp / (float)V;
            o[plane] = (float)cr / (float)V;
            o[2 * plane] = cp + cr ? 2.f * (float)cp * (float)cr / ((float)V * (float)(cp + cr)) : 0.f;      // = 2 P R / (P + R), one rounding
        }
        if (tid == 64) err[r] = (((red_e[0] + red_e[1]) + red_e[2]) + red_e[3]) / (float)V;
    }
}

}}  // namespace mhe::mesh_eval

using namespace mhe;

extern "C" int mhe_mesh_eval_f32(const float *pred, const float *target, const float *scale, const float *thr, float *err, float *prf, int N, int B, int V,
                                 int T, float unit, void *stream) {
    MHE_REQUIRE(pred && target && scale && thr && err && prf, "mhe_mesh_eval_f32: null pointer");
    MHE_REQUIRE(N > 0 && B > 0, "mhe_mesh_eval_f32: N=%d B=%d", N, B);
    MHE_REQUIRE(V >= 1 && V <= mesh_eval::VMAX, "mhe_mesh_eval_f32: V=%d (V in 1..%d)", V, mesh_eval::VMAX);
    MHE_REQUIRE(T >= 1 && T <= mesh_eval::TMAX, "mhe_mesh_eval_f32: T=%d (T in 1..%d)", T, mesh_eval::TMAX);
    MHE_REQUIRE((long)N * B <= 0x7fffffffL, "mhe_mesh_eval_f32: N*B=%ld rows (at most 2^31 - 1)", (long)N * B);
    MHE_REQUIRE(unit == unit, "mhe_mesh_eval_f32: unit is NaN");
    mesh_eval::Thr th;
    th.T = T;
    for (int t = 0; t < mesh_eval::TMAX; ++t) {
        th.v[t] = t < T ? thr[t] : 0.f;
        MHE_REQUIRE(th.v[t] == th.v[t], "mhe_mesh_eval_f32: thr[%d] is NaN", t);
    }
    const size_t R = (size_t)N * B;
    struct { const void *p; size_t n; } in[3] = {{pred, R * V * 12}, {target, (size_t)B * V * 12}, {scale, (size_t)B * 4}},
                                        out[2] = {{err, R * 4}, {prf, R * T * 12}};
    for (int o = 0; o < 2; ++o)
        for (int i = 0; i < 3; ++i) MHE_REQUIRE(disjoint(out[o].p, out[o].n, in[i].p, in[i].n), "mhe_mesh_eval_f32: output %d overlaps input %d", o, i);
    MHE_REQUIRE(disjoint(err, R * 4, prf, R * T * 12), "mhe_mesh_eval_f32: err and prf overlap");
    // hypotheses per workgroup: as few as it takes to reach WG_TARGET workgroups (staging the target is V loads against the V^2 pairs of a hypothesis)
    int chunks = std::min(N, (mesh_eval::WG_TARGET + B - 1) / B);
    const int G = (N + chunks - 1) / chunks;
    chunks = (N + G - 1) / G;
    const dim3 grid((unsigned)((size_t)B * chunks));
    switch ((V + mesh_eval::NT - 1) / mesh_eval::NT) {
#define MHE_CASE(K)                                                                                                                                   \
    case K:                                                                                                                                           \
        hipLaunchKernelGGL(mesh_eval::mesh_eval_kernel<K>, grid, dim3(mesh_eval::NT), 0, (hipStream_t)stream, pred, target, scale, err, prf, N, B, V, G, \
                           chunks, unit, th);                                                                                                         \
        break;
        MHE_CASE(1) MHE_CASE(2) MHE_CASE(3) MHE_CASE(4)
#undef MHE_CASE
    }
    return check_launch("mesh_eval_kernel");
}
