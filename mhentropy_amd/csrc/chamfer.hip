// Hand-object Chamfer distance (reference hand/criteria.py:18-39) and its reverse (criteria.chamfer_dist, ops.chamfer / ops.chamfer_bwd).
//   a_j = p_j (scale[b] unit) + root[b],  D1 = mean_j min_v |a_j - o_v|,  D2 = mean_{v < V_b} min_j |a_j - o_v|,  dist = D1 + D2
// without the reference's (N, B, P, VO) tensor.  f32, squared distances compared and one square root per minimum, ties to the lowest index,
// fixed summation order and no atomics in either direction: two launches give the same bits.
#include <algorithm>
#include "common.h"

namespace mhe { namespace chamfer {

constexpr int NT = 256;                    // threads of a workgroup
constexpr int TV = 1024, KV = TV / NT;     // object vertices of one LDS tile; of one thread
constexpr int KP = 8, ITEMS = NT * KP;     // hand points ((hypothesis, joint) pairs) of one thread; of one workgroup
constexpr int GMAX = 128;                  // hypotheses of one workgroup
constexpr int PMAX = MHE_CHAMFER_MAX_POINTS;

__device__ __forceinline__ float sqdist(float ax, float ay, float az, const float4 &o) {
    const float dx = ax - o.x, dy = ay - o.y, dz = az - o.z;
    return fmaf(dz, dz, fmaf(dy, dy, dx * dx));
}

// min over the tile's tv vertices for K hand points held in registers: every lane reads the same vertex (an LDS broadcast), one read serves K pairs
template <bool IDX, int K>
__device__ __forceinline__ void scan_vertices(const float4 *tile, int tv, int t0, const float *ax, const float *ay, const float *az, float *m, int *mi) {
#pragma unroll 4
    for (int v = 0; v < tv; ++v) {
        const float4 o = tile[v];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const float d = sqdist(ax[k], ay[k], az[k], o);
            if (IDX) { if (d < m[k]) { m[k] = d; mi[k] = t0 + v; } }
            else m[k] = fminf(m[k], d);
        }
    }
}

// min over one hypothesis' P hand points for K object vertices held in registers
template <bool IDX, int K>
__device__ __forceinline__ void scan_points(const float4 *hand, int P, const float4 *o, float *m, int *mi) {
#pragma unroll
    for (int k = 0; k < K; ++k) { m[k] = __builtin_inff(); mi[k] = 0; }
#pragma unroll 4
    for (int j = 0; j < P; ++j) {
        const float4 h = hand[j];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const float d = sqdist(h.x, h.y, h.z, o[k]);
            if (IDX) { if (d < m[k]) { m[k] = d; mi[k] = j; } }
            else m[k] = fminf(m[k], d);
        }
    }
}

// Workgroup (b, c): image b, hypotheses n0 .. n0 + g - 1 (g <= G, g P <= ITEMS).  The image's vertices come from HBM once, tile by tile, and
// every tile serves all g hypotheses from LDS, in both directions:
//   hand -> object: a thread keeps up to KP hand points and their running (min, argmin) in registers across the tiles;
//   object -> hand: a thread keeps up to KV vertices of the tile, walks a hypothesis' hand points (LDS, broadcast) and the wave adds the square
//   roots by its butterfly; wave w's partial sum of hypothesis n lives in d2w[n][w] and grows tile by tile.
// Vertices at or past V_b are never loaded; with obj_count NULL V_b = VO and nothing is paid for the option.
template <bool IDX>
__global__ __launch_bounds__(NT) void chamfer_fwd_kernel(const float *__restrict__ points, const float *__restrict__ scale, const float *__restrict__ root,
                                                         const float *__restrict__ obj, const int *__restrict__ obj_count, float *__restrict__ dist,
                                                         float *__restrict__ parts, int *__restrict__ idx_p, int *__restrict__ idx_o, int N, int B, int P,
                                                         int VO, int G, int chunks, float unit) {
    __shared__ float4 hand[ITEMS];          // (a_j, then its distance in .w), item = n_local P + j
    __shared__ float4 tile[TV];
    __shared__ float d2w[GMAX][NT / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.x / chunks, n0 = (blockIdx.x % chunks) * G;
    const int g = min(G, N - n0), items = g * P, nk = (items + NT - 1) / NT;
    const int Vb = obj_count ? min(max(obj_count[b], 1), VO) : VO;
    const float su = scale[b] * unit, rx = root[(size_t)b * 3], ry = root[(size_t)b * 3 + 1], rz = root[(size_t)b * 3 + 2];

    float ax[KP], ay[KP], az[KP], m1[KP];
    int i1[KP];
#pragma unroll
    for (int k = 0; k < KP; ++k) {
        const int item = k * NT + tid;
        ax[k] = ay[k] = az[k] = 0.f;
        m1[k] = __builtin_inff();
        i1[k] = 0;
        if (item < items) {
            const int n = item / P, j = item - n * P;
            const float *p = points + (((size_t)(n0 + n) * B + b) * P + j) * 3;
            ax[k] = fmaf(p[0], su, rx); ay[k] = fmaf(p[1], su, ry); az[k] = fmaf(p[2], su, rz);
            hand[item] = make_float4(ax[k], ay[k], az[k], 0.f);
        }
    }

    for (int t0 = 0; t0 < Vb; t0 += TV) {
        const int tv = min(TV, Vb - t0), nkv = (tv + NT - 1) / NT;
        __syncthreads();                                           // the previous tile is done with; (first pass: hand[] is written)
        for (int v = tid; v < tv; v += NT) {
            const float *o = obj + ((size_t)b * VO + t0 + v) * 3;
            tile[v] = make_float4(o[0], o[1], o[2], 0.f);
        }
        __syncthreads();
        switch (nk) {
#define MHE_CASE(K) case K: scan_vertices<IDX, K>(tile, tv, t0, ax, ay, az, m1, i1); break;
            MHE_CASE(1) MHE_CASE(2) MHE_CASE(3) MHE_CASE(4) MHE_CASE(5) MHE_CASE(6) MHE_CASE(7) MHE_CASE(8)
#undef MHE_CASE
        }
        float4 o[KV];
#pragma unroll
        for (int k = 0; k < KV; ++k) o[k] = k * NT + tid < tv ? tile[k * NT + tid] : make_float4(0.f, 0.f, 0.f, 0.f);
        for (int n = 0; n < g; ++n) {
            float m2[KV];
            int i2[KV];
            switch (nkv) {
#define MHE_CASE(K) case K: scan_points<IDX, K>(hand + n * P, P, o, m2, i2); break;
                MHE_CASE(1) MHE_CASE(2) MHE_CASE(3) MHE_CASE(4)
#undef MHE_CASE
            }
            float s = 0.f;
#pragma unroll
            for (int k = 0; k < KV; ++k)
                if (k < nkv && k * NT + tid < tv) {
                    s += sqrtf(m2[k]);
                    if (IDX && idx_o) idx_o[((size_t)(n0 + n) * B + b) * VO + t0 + k * NT + tid] = i2[k];
                }
            s = wave_sum(s);
            if (lane == 0) d2w[n][wave] = t0 ? d2w[n][wave] + s : s;
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < KP; ++k) {
        const int item = k * NT + tid;
        if (item < items) {
            hand[item].w = sqrtf(m1[k]);
            if (IDX && idx_p) {
                const int n = item / P, j = item - n * P;
                idx_p[((size_t)(n0 + n) * B + b) * P + j] = i1[k];
            }
        }
    }
    __syncthreads();
    for (int n = wave; n < g; n += NT / 64) {
        float s = 0.f;
        for (int j = lane; j < P; j += 64) s += hand[n * P + j].w;
        s = wave_sum(s);
        if (lane == 0) {
            const size_t r = (size_t)(n0 + n) * B + b;
            const float D1 = s / (float)P, D2 = (((d2w[n][0] + d2w[n][1]) + d2w[n][2]) + d2w[n][3]) / (float)Vb;
            dist[r] = D1 + D2;
            if (parts) { parts[r * 2] = D1; parts[r * 2 + 1] = D2; }
        }
    }
    if (IDX && idx_o && Vb < VO)
        for (int n = 0; n < g; ++n)
            for (int v = Vb + tid; v < VO; v += NT) idx_o[((size_t)(n0 + n) * B + b) * VO + v] = -1;
}

constexpr int TB = 2048;                   // idx_o entries of one LDS tile of the reverse

// Reverse, one workgroup per row r.  Hand point j gathers its own object vertices (idx_o[r][v] == j): S = NT / min(P, NT) threads share a hand
// point, thread (j, s) walks the s-th part of every tile of idx_o in ascending v, and the S partial sums are added in ascending s - a fixed
// order, no atomics.  P > NT: rounds of NT hand points.  u(0) = 0; an idx_p outside 0 .. V_b - 1 contributes nothing (it is never dereferenced).
__global__ __launch_bounds__(NT) void chamfer_bwd_kernel(const float *__restrict__ points, const float *__restrict__ scale, const float *__restrict__ root,
                                                         const float *__restrict__ obj, const int *__restrict__ obj_count, const int *__restrict__ idx_p,
                                                         const int *__restrict__ idx_o, const float *__restrict__ g_dist, float *__restrict__ g_points,
                                                         int B, int P, int VO, float unit) {
    __shared__ int ti[TB];
    __shared__ float part[3][NT];
    const int tid = threadIdx.x;
    const size_t r = blockIdx.x;
    const int b = (int)(r % (size_t)B);
    const int Vb = obj_count ? min(max(obj_count[b], 1), VO) : VO;
    const float su = scale[b] * unit, rx = root[(size_t)b * 3], ry = root[(size_t)b * 3 + 1], rz = root[(size_t)b * 3 + 2];
    const int JR = min(P, NT), S = NT / JR, s = tid / JR, jl = tid - s * JR;
    const float *ob = obj + (size_t)b * VO * 3;
    for (int j0 = 0; j0 < P; j0 += JR) {
        const int j = j0 + jl;
        const bool valid = s < S && j < P;
        float ax = 0.f, ay = 0.f, az = 0.f, gx = 0.f, gy = 0.f, gz = 0.f;
        if (valid) {
            const float *p = points + (r * P + j) * 3;
            ax = fmaf(p[0], su, rx); ay = fmaf(p[1], su, ry); az = fmaf(p[2], su, rz);
        }
        for (int t0 = 0; t0 < Vb; t0 += TB) {
            const int tv = min(TB, Vb - t0), ct = (tv + S - 1) / S;
            __syncthreads();
            for (int v = tid; v < tv; v += NT) ti[v] = idx_o[r * VO + t0 + v];
            __syncthreads();
            if (valid) {
                const int hi = min(tv, (s + 1) * ct);
                for (int v = s * ct; v < hi; ++v)
                    if (ti[v] == j) {
                        const float *o = ob + (size_t)(t0 + v) * 3;
                        const float dx = ax - o[0], dy = ay - o[1], dz = az - o[2], q = fmaf(dz, dz, fmaf(dy, dy, dx * dx));
                        if (q > 0.f) {
                            const float inv = 1.f / sqrtf(q);
                            gx = fmaf(dx, inv, gx); gy = fmaf(dy, inv, gy); gz = fmaf(dz, inv, gz);
                        }
                    }
            }
        }
        part[0][tid] = gx; part[1][tid] = gy; part[2][tid] = gz;
        __syncthreads();
        if (valid && s == 0) {
            for (int q = 1; q < S; ++q) { gx += part[0][q * JR + jl]; gy += part[1][q * JR + jl]; gz += part[2][q * JR + jl]; }
            float ux = 0.f, uy = 0.f, uz = 0.f;
            const int ip = idx_p[r * P + j];
            if ((unsigned)ip < (unsigned)Vb) {
                const float *o = ob + (size_t)ip * 3;
                const float dx = ax - o[0], dy = ay - o[1], dz = az - o[2], q = fmaf(dz, dz, fmaf(dy, dy, dx * dx));
                if (q > 0.f) {
                    const float inv = 1.f / sqrtf(q);
                    ux = dx * inv; uy = dy * inv; uz = dz * inv;
                }
            }
            const float c = g_dist[r] * su, ip_ = 1.f / (float)P, iv = 1.f / (float)Vb;
            float *gp = g_points + (r * P + j) * 3;
            gp[0] = c * fmaf(ux, ip_, gx * iv); gp[1] = c * fmaf(uy, ip_, gy * iv); gp[2] = c * fmaf(uz, ip_, gz * iv);
        }
    }
}

}}  // namespace mhe::chamfer

using namespace mhe;

// the shared argument checks of both entries; R = N B rows
static int chamfer_args(const char *who, const void *points, const void *scale, const void *root, const void *obj, int N, int B, int P, int VO, float unit) {
    MHE_REQUIRE(points && scale && root && obj, "%s: null pointer", who);
    MHE_REQUIRE(N > 0 && B > 0, "%s: N=%d B=%d", who, N, B);
    MHE_REQUIRE(P >= 1 && P <= chamfer::PMAX, "%s: P=%d (P in 1..%d)", who, P, chamfer::PMAX);
    MHE_REQUIRE(VO >= 1, "%s: VO=%d (VO >= 1)", who, VO);
    MHE_REQUIRE((long)N * B <= 0x7fffffffL, "%s: N*B=%ld rows (at most 2^31 - 1)", who, (long)N * B);
    MHE_REQUIRE(unit == unit, "%s: unit is NaN", who);
    return MHE_OK;
}

extern "C" int mhe_chamfer_f32(const float *points, const float *scale, const float *root, const float *obj, const int *obj_count, float *dist, float *parts,
                               int *idx_p, int *idx_o, int N, int B, int P, int VO, float unit, void *stream) {
    if (int st = chamfer_args("mhe_chamfer_f32", points, scale, root, obj, N, B, P, VO, unit)) return st;
    MHE_REQUIRE(dist, "mhe_chamfer_f32: null pointer (dist)");
    const size_t R = (size_t)N * B;
    struct { const void *p; size_t n; } in[5] = {{points, R * P * 12}, {scale, (size_t)B * 4}, {root, (size_t)B * 12}, {obj, (size_t)B * VO * 12},
                                                 {obj_count, (size_t)B * 4}},
                                        out[4] = {{dist, R * 4}, {parts, R * 8}, {idx_p, R * P * 4}, {idx_o, R * VO * 4}};
    for (int o = 0; o < 4; ++o) {
        for (int i = 0; i < 5; ++i)
            MHE_REQUIRE(disjoint(out[o].p, out[o].n, in[i].p, in[i].n), "mhe_chamfer_f32: output %d overlaps input %d", o, i);
        for (int q = 0; q < o; ++q) MHE_REQUIRE(disjoint(out[o].p, out[o].n, out[q].p, out[q].n), "mhe_chamfer_f32: outputs %d and %d overlap", q, o);
    }
    // hypotheses per workgroup: what its registers and LDS hold, fewer where that leaves the chip short of workgroups
    const int gmax = std::min(N, std::min(chamfer::GMAX, chamfer::ITEMS / P));
    int chunks = std::min(N, std::max((N + gmax - 1) / gmax, (512 + B - 1) / B));
    const int G = (N + chunks - 1) / chunks;
    chunks = (N + G - 1) / G;
    const dim3 grid((unsigned)((size_t)B * chunks));
    if (idx_p || idx_o)
        hipLaunchKernelGGL(chamfer::chamfer_fwd_kernel<true>, grid, dim3(chamfer::NT), 0, (hipStream_t)stream, points, scale, root, obj, obj_count, dist, parts,
                           idx_p, idx_o, N, B, P, VO, G, chunks, unit);
    else
        hipLaunchKernelGGL(chamfer::chamfer_fwd_kernel<false>, grid, dim3(chamfer::NT), 0, (hipStream_t)stream, points, scale, root, obj, obj_count, dist, parts,
                           idx_p, idx_o, N, B, P, VO, G, chunks, unit);
    return check_launch("chamfer_fwd_kernel");
}

extern "C" int mhe_chamfer_bwd_f32(const float *points, const float *scale, const float *root, const float *obj, const int *obj_count, const int *idx_p,
                                   const int *idx_o, const float *g_dist, float *g_points, int N, int B, int P, int VO, float unit, void *stream) {
    if (int st = chamfer_args("mhe_chamfer_bwd_f32", points, scale, root, obj, N, B, P, VO, unit)) return st;
    MHE_REQUIRE(idx_p && idx_o && g_dist && g_points, "mhe_chamfer_bwd_f32: null pointer (idx_p, idx_o, g_dist, g_points)");
    const size_t R = (size_t)N * B;
    struct { const void *p; size_t n; } in[8] = {{points, R * P * 12}, {scale, (size_t)B * 4}, {root, (size_t)B * 12}, {obj, (size_t)B * VO * 12},
                                                 {obj_count, (size_t)B * 4}, {idx_p, R * P * 4}, {idx_o, R * VO * 4}, {g_dist, R * 4}};
    for (int i = 0; i < 8; ++i) MHE_REQUIRE(disjoint(g_points, R * P * 12, in[i].p, in[i].n), "mhe_chamfer_bwd_f32: g_points overlaps input %d", i);
    hipLaunchKernelGGL(chamfer::chamfer_bwd_kernel, dim3((unsigned)R), dim3(chamfer::NT), 0, (hipStream_t)stream, points, scale, root, obj, obj_count, idx_p,
                       idx_o, g_dist, g_points, B, P, VO, unit);
    return check_launch("chamfer_bwd_kernel");
}
