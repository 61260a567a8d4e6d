// Evaluation reductions of the body head (body.point_errors, body.min_of_n; the protocol of BodyFlowHead.evaluate): the mean point distance of
// every hypothesis to its image's target, and the minimum over the first n hypotheses of an image for a list of n.  Inference only, f32, fixed
// summation order, no atomics: two launches give the same bits.
#include "common.h"

namespace mhe { namespace body {

// err[b][k] = mean_p || (points[b][k][p] - mean_{q in root} points[b][k][q]) - (target[b][p] - mean_{q in root} target[b][q]) ||, P <= 64: one
// wave per row, lane p holds point p; the root means are summed in index order by every lane alike (uniform loads), the P distances by the
// wave's butterfly (lanes past P add 0).  root_mask = 0: no centring.
__global__ __launch_bounds__(256) void point_errors_kernel(const float *__restrict__ pts, const float *__restrict__ tgt, float *__restrict__ err, long R, int K,
                                                           int P, unsigned long long root_mask) {
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= R) return;
    const float *p = pts + (size_t)row * P * 3, *t = tgt + (size_t)(row / K) * P * 3;
    float pr[3] = {0.f, 0.f, 0.f}, tr[3] = {0.f, 0.f, 0.f};
    if (root_mask) {
        int n = 0;
        for (int q = 0; q < P; ++q)
            if ((root_mask >> q) & 1) {
#pragma unroll
                for (int c = 0; c < 3; ++c) { pr[c] += p[q * 3 + c]; tr[c] += t[q * 3 + c]; }
                ++n;
            }
#pragma unroll
        for (int c = 0; c < 3; ++c) { pr[c] /= (float)n; tr[c] /= (float)n; }
    }
    float d = 0.f;
    if (lane < P) {
        float sq = 0.f;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float e = (p[lane * 3 + c] - pr[c]) - (t[lane * 3 + c] - tr[c]);
            sq = fmaf(e, e, sq);
        }
        d = sqrtf(sq);
    }
    d = wave_sum(d);
    if (lane == 0) err[row] = d / (float)P;
}

struct MinNs { int n, ns[8]; };

// values[b][i] = min err[b][0 .. ns[i] - 1], index[b][i] = the lowest k that attains it; ns strictly increasing.  One wave per image: the lanes
// walk the segment [ns[i-1], ns[i]) with their running (value, index), then the wave's butterfly picks the smaller value, the lower index on a tie.
__global__ __launch_bounds__(256) void min_of_n_kernel(const float *__restrict__ err, float *__restrict__ val, int *__restrict__ idx, int B, int K, MinNs m) {
    const int b = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (b >= B) return;
    const float *e = err + (size_t)b * K;
    float cv = __builtin_inff();
    int ck = 0x7fffffff, lo = 0;
    for (int i = 0; i < m.n; ++i) {
        for (int k = lo + lane; k < m.ns[i]; k += 64) {
            const float v = e[k];
            if (v < cv || (v == cv && k < ck)) { cv = v; ck = k; }
        }
        lo = m.ns[i];
        float rv = cv;
        int rk = ck;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ov = __shfl_xor(rv, o, 64);
            const int ok = __shfl_xor(rk, o, 64);
            if (ov < rv || (ov == rv && ok < rk)) { rv = ov; rk = ok; }
        }
        if (lane == 0) {
            val[(size_t)b * m.n + i] = rv;
            idx[(size_t)b * m.n + i] = rk == 0x7fffffff ? 0 : rk;          // (only non-finite input leaves no index: unspecified, but in range)
        }
    }
}

}}  // namespace mhe::body

using namespace mhe;

extern "C" int mhe_point_errors_f32(const float *points, const float *target, float *err, int B, int K, int P, unsigned long long root_mask,
                                    void *stream) {
    MHE_REQUIRE(points && target && err, "mhe_point_errors_f32: null pointer");
    MHE_REQUIRE(B > 0 && K > 0 && P >= 1 && P <= 64, "mhe_point_errors_f32: B=%d K=%d P=%d (P in 1..64)", B, K, P);
    MHE_REQUIRE(P == 64 || (root_mask >> P) == 0, "mhe_point_errors_f32: a root index is outside 0..%d", P - 1);
    const long R = (long)B * K;
    hipLaunchKernelGGL(body::point_errors_kernel, dim3((unsigned)((R + 3) / 4)), dim3(256), 0, (hipStream_t)stream, points, target, err, R, K, P, root_mask);
    return check_launch("point_errors_kernel");
}

extern "C" int mhe_min_of_n_f32(const float *err, float *values, int *index, int B, int K, const int *ns, int n, void *stream) {
    MHE_REQUIRE(n >= 1 && n <= 8 && ns, "mhe_min_of_n_f32: n=%d outside 1..8 (or ns null; ns is host memory)", n);
    MHE_REQUIRE(B > 0 && K > 0, "mhe_min_of_n_f32: B=%d K=%d", B, K);
    body::MinNs m;
    m.n = n;
    for (int i = 0; i < 8; ++i) m.ns[i] = i < n ? ns[i] : 0;
    for (int i = 0; i < n; ++i)
        MHE_REQUIRE(ns[i] >= 1 && ns[i] <= K && (i == 0 || ns[i] > ns[i - 1]), "mhe_min_of_n_f32: ns must be strictly increasing in 1..K=%d (ns[%d]=%d)", K,
                    i, ns[i]);
    MHE_REQUIRE(err && values && index, "mhe_min_of_n_f32: null pointer");
    hipLaunchKernelGGL(body::min_of_n_kernel, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, (hipStream_t)stream, err, values, index, B, K, m);
    return check_launch("min_of_n_kernel");
}
