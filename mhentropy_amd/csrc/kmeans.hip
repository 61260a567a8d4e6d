// k-means quantisation of a hypothesis set (the n-quantised-best-of-M protocol: draw M samples, cluster them into n modes, report the
// modes): per image the N points [N,B,D] are clustered into Q groups by farthest-point seeding and Lloyd iterations, each cluster is
// reported by the member nearest its mean, and the clusters come out largest first.  One workgroup per image; the image's points, the
// centres and the per-point assignment and distance stay in LDS for the whole call (one launch instead of a cdist / argmin / index_add
// loop per iteration).  DESIGN.md, "k-means quantisation", has the algorithm with its tie rules; they are fixed so that a float64
// restatement (tests/kmeans_ref.py) takes the same decisions:
//   distance   sum over d, ascending, of (p_d - c_d)^2 in f32 (one fused multiply-add per d; never the expanded |p|^2 - 2 p.c + |c|^2)
//   seeds      0: highest score, ties to the lower n (no score: n = 0); k: farthest from its nearest earlier seed, ties to the lower n
//   assign     nearest centre, ties to the lower k
//   mean       serial f32 sum over the members in ascending n, one division; an empty cluster keeps its centre
//   member     nearest its centre, ties to the lower n; an empty cluster: nearest among all N, count 0
//   order      count descending, ties to the lower representative, then to the lower seed slot
// Every index the kernel forms comes out of a comparison whose fall-back is a valid index, so NaN / Inf coordinates or scores give
// unspecified clusters but no access outside the image's rows (a NaN score counts as -Inf, a NaN distance as the worst of its search).
// Sums have a fixed order and there is no atomic: two calls give the same bits.
#include <climits>
#include "common.h"

namespace mhe { namespace kmeans {

constexpr int THREADS = 256, WAVES = THREADS / 64;
constexpr int SCRATCH = 16;                         // words: the block reduction's [WAVES] values and [WAVES] indices, the "changed" flag
constexpr size_t LDS_LIMIT = 160 * 1024;            // the LDS of one gfx950 CU, all of which one workgroup may take

// rows of points and centres are D | 1 words apart: an odd stride puts the rows of the 32 lanes of an LDS lane group on 32 banks
__host__ __device__ __forceinline__ int row_stride(int D) { return D | 1; }
// points [N][Ds], centres [Q][Ds], distance [N], assignment [N], count / representative / slot [Q], scratch
static inline size_t lds_words(int N, int Q, int D) {
    return ((size_t)N + (size_t)Q) * (size_t)row_stride(D) + 2 * (size_t)N + 3 * (size_t)Q + SCRATCH;
}

__device__ __forceinline__ float sqdist(const float *p, const float *c, int D) {
    float e = 0.f;
    for (int d = 0; d < D; ++d) { const float df = p[d] - c[d]; e = fmaf(df, df, e); }
    return e;
}

// the greater of (v, i) and (ov, oi): higher value, ties to the lower index
__device__ __forceinline__ void keep_best(float &v, int &i, float ov, int oi) {
    if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
}
__device__ __forceinline__ void wave_best(float &v, int &i) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(v, o, 64);
        const int oi = __shfl_xor(i, o, 64);
        keep_best(v, i, ov, oi);
    }
}
// index of the highest value over the workgroup, ties to the lower index; a thread with nothing to offer passes (-inf, INT_MAX)
__device__ __forceinline__ int block_best(float v, int i, float *redv, int *redi) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    wave_best(v, i);
    if (lane == 0) { redv[wave] = v; redi[wave] = i; }
    __syncthreads();
    v = redv[0]; i = redi[0];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) keep_best(v, i, redv[w], redi[w]);
    __syncthreads();                                // the scratch is free again
    return i;
}

// point p's nearest centre (ties to the lower k) and its squared distance; four centres share one read of the point
__device__ __forceinline__ void nearest(const float *p, const float *ctr, int Q, int D, int Ds, float &bd, int &bk) {
    bd = 0.f; bk = 0;
    for (int k0 = 0; k0 < Q; k0 += 4) {
        const float *c0 = ctr + (size_t)k0 * Ds;
        const float *c1 = ctr + (size_t)(k0 + 1 < Q ? k0 + 1 : k0) * Ds;
        const float *c2 = ctr + (size_t)(k0 + 2 < Q ? k0 + 2 : k0) * Ds;
        const float *c3 = ctr + (size_t)(k0 + 3 < Q ? k0 + 3 : k0) * Ds;
        float e[4] = {0.f, 0.f, 0.f, 0.f};
        for (int d = 0; d < D; ++d) {
            const float x = p[d];
            const float d0 = x - c0[d], d1 = x - c1[d], d2 = x - c2[d], d3 = x - c3[d];
            e[0] = fmaf(d0, d0, e[0]); e[1] = fmaf(d1, d1, e[1]); e[2] = fmaf(d2, d2, e[2]); e[3] = fmaf(d3, d3, e[3]);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (k0 + j < Q && (k0 + j == 0 || e[j] < bd)) { bd = e[j]; bk = k0 + j; }
    }
}

__global__ __launch_bounds__(THREADS) void kmeans_kernel(const float *__restrict__ points, const float *__restrict__ score,
                                                         int *__restrict__ index, int *__restrict__ count, int *__restrict__ assign,
                                                         float *__restrict__ centre, int *__restrict__ converged, int N, int B, int D,
                                                         int Q, int iters) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int b = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, Ds = row_stride(D);
    const float INF = __builtin_inff();
    float *pts = lds, *ctr = pts + (size_t)N * Ds, *dist = ctr + (size_t)Q * Ds;
    int *asg = reinterpret_cast<int *>(dist + N), *cnt = asg + N, *rep = cnt + Q, *slot = rep + Q;
    float *redv = reinterpret_cast<float *>(slot + Q);
    int *redi = reinterpret_cast<int *>(redv + WAVES);
    int *flag = redi + WAVES;                        // "an assignment changed": a word of the scratch, not __syncthreads_or - the library's
                                                     // workgroup reduction brings 256 bytes of static LDS that the budget would not count

    for (int i = tid; i < N * D; i += THREADS) {     // (N * D is below the LDS limit's 40,960 words)
        const int n = i / D, d = i - n * D;
        pts[n * Ds + d] = points[((size_t)n * B + b) * D + d];
    }
    for (int n = tid; n < N; n += THREADS) asg[n] = -1;

    // ---- seeding by farthest-point traversal; dist[n] is point n's distance to its nearest seed so far (thread-private until the loop ends)
    int seed = 0;
    if (score) {                                     // (uniform over the workgroup)
        float bv = -INF; int bi = INT_MAX;
        for (int n = tid; n < N; n += THREADS) {
            float s = score[(size_t)n * B + b];
            s = s == s ? s : -INF;
            if (bi == INT_MAX || s > bv) { bv = s; bi = n; }
        }
        seed = block_best(bv, bi, redv, redi);
    }
    __syncthreads();                                 // the points are in
    for (int k = 0; k < Q; ++k) {
        if (k > 0) {
            float bv = -INF; int bi = INT_MAX;
            for (int n = tid; n < N; n += THREADS) {
                float v = dist[n];
                v = v == v ? v : -INF;
                if (bi == INT_MAX || v > bv) { bv = v; bi = n; }
            }
            seed = block_best(bv, bi, redv, redi);
        }
        for (int d = tid; d < D; d += THREADS) ctr[k * Ds + d] = pts[seed * Ds + d];
        __syncthreads();
        if (k + 1 < Q)
            for (int n = tid; n < N; n += THREADS) {
                const float e = sqdist(pts + n * Ds, ctr + k * Ds, D);
                dist[n] = k == 0 ? e : fminf(dist[n], e);
            }
    }

    // ---- Lloyd: at most `iters` rounds of (assign, stop at a fixed point, means); without a fixed point one more assignment follows the
    // last means, so that assign / dist always belong to the centres returned
    int conv = 0;
    for (int it = 0; it <= iters && !conv; ++it) {
        int changed = 0;
        if (tid == 0) *flag = 0;
        __syncthreads();
        for (int n = tid; n < N; n += THREADS) {
            float bd; int bk;
            nearest(pts + n * Ds, ctr, Q, D, Ds, bd, bk);
            changed |= bk != asg[n];
            asg[n] = bk; dist[n] = bd;
        }
        if (changed) *flag = 1;
        __syncthreads();
        changed = *flag;                             // (reset only after the barrier that ends the round, or never again)
        if (it == iters) break;
        if (it > 0 && !changed) { conv = 1; break; }  // (the first round always counts as changed: asg was -1)
        for (int i = tid; i < Q * D; i += THREADS) {  // one thread per (cluster, coordinate): the members in ascending n
            const int k = i / D, d = i - k * D;
            float s = 0.f; int c = 0;
            for (int n = 0; n < N; ++n)
                if (asg[n] == k) { s += pts[n * Ds + d]; ++c; }
            if (c > 0) ctr[k * Ds + d] = s / (float)c;
        }
        __syncthreads();
    }

    // ---- sizes and representatives: one wave per cluster
    for (int k = wave; k < Q; k += WAVES) {
        int c = 0;
        for (int n = lane; n < N; n += 64) c += asg[n] == k ? 1 : 0;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
        float bv = -INF; int bi = INT_MAX;
        for (int n = lane; n < N; n += 64) {
            if (c != 0 && asg[n] != k) continue;
            float e = c == 0 ? sqdist(pts + n * Ds, ctr + k * Ds, D) : dist[n];
            e = e == e ? -e : -INF;
            if (bi == INT_MAX || e > bv) { bv = e; bi = n; }
        }
        wave_best(bv, bi);
        if (lane == 0) { cnt[k] = c; rep[k] = bi; }
    }
    __syncthreads();

    // ---- output order: rank by counting
    for (int k = tid; k < Q; k += THREADS) {
        const int c = cnt[k], r = rep[k];
        int rank = 0;
        for (int j = 0; j < Q; ++j) {
            const int cj = cnt[j], rj = rep[j];
            rank += (cj > c || (cj == c && (rj < r || (rj == r && j < k)))) ? 1 : 0;
        }
        slot[k] = rank;
        index[(size_t)rank * B + b] = r;
        count[(size_t)rank * B + b] = c;
    }
    __syncthreads();
    for (int i = tid; i < Q * D; i += THREADS) {
        const int k = i / D, d = i - k * D;
        centre[((size_t)slot[k] * B + b) * D + d] = ctr[k * Ds + d];
    }
    for (int n = tid; n < N; n += THREADS) assign[(size_t)n * B + b] = slot[asg[n]];
    if (tid == 0) converged[b] = conv;
}

}}  // namespace mhe::kmeans

using namespace mhe;

extern "C" size_t mhe_kmeans_lds_limit(void) { return kmeans::LDS_LIMIT; }

extern "C" size_t mhe_kmeans_lds_bytes(int N, int Q, int D) {
    if (N <= 0 || Q <= 0 || D <= 0) return 0;
    return kmeans::lds_words(N, Q, D) * sizeof(float);
}

extern "C" int mhe_kmeans_select_f32(const float *points, const float *score, int *index, int *count, int *assign, float *centre,
                                     int *converged, int N, int B, int D, int Q, int iters, void *stream) {
    MHE_REQUIRE(points && index && count && assign && centre && converged, "mhe_kmeans_select_f32: null pointer");
    MHE_REQUIRE(N > 0 && B > 0 && D > 0 && Q > 0 && Q <= N && iters >= 0, "mhe_kmeans_select_f32: need 0 < Q <= N, 0 < B, D and 0 <= iters (N=%d B=%d D=%d Q=%d iters=%d)",
                N, B, D, Q, iters);
    const size_t need = mhe_kmeans_lds_bytes(N, Q, D);
    MHE_REQUIRE(need <= kmeans::LDS_LIMIT, "mhe_kmeans_select_f32: N=%d Q=%d D=%d needs %zu bytes of LDS, over the %zu (160 KiB) of one CU: there is no "
                "slower path", N, Q, D, need, kmeans::LDS_LIMIT);
    MHE_REQUIRE(on_device(points) && (!score || on_device(score)) && on_device(index) && on_device(count) && on_device(assign) && on_device(centre) &&
                on_device(converged), "mhe_kmeans_select_f32: every pointer must be device memory");
    // the kernel has no static LDS, so `need` is all it takes; a runtime that does not grant it must not see the launch
    const hipError_t grant = hipFuncSetAttribute(reinterpret_cast<const void *>(kmeans::kmeans_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)need);
    if (grant != hipSuccess) {
        (void)hipGetLastError();
        set_error("mhe_kmeans_select_f32: the runtime does not grant %zu bytes of LDS to one workgroup (%s)", need, hipGetErrorString(grant));
        return MHE_ERR_LAUNCH;
    }
    hipLaunchKernelGGL(kmeans::kmeans_kernel, dim3(B), dim3(kmeans::THREADS), need, (hipStream_t)stream, points, score, index, count, assign,
                       centre, converged, N, B, D, Q, iters);
    return check_launch("kmeans_kernel");
}
