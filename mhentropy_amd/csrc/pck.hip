// 3D PCK curve and its area (criteria.pck_auc, ops.pck_curve): for every hypothesis the number of valid points whose distance to the image's
// ground truth is at most each of T thresholds, the trapezoid area under that curve and the mean distance, without a per-point distance tensor.
//   su = scale[b] unit,  p = pred[r] su,  g = target[b] su,  d_p = |p - g|  (f32)
//   hits[r][i] = #{valid p: d_p <= thr[i]}                                   (inclusive, integers)
//   err[r]     = (1/n_valid) sum over the valid p of d_p                     (fixed order)
//   auc[r]     = sum_{i<T-1} (thr[i+1] - thr[i]) (hits[i] + hits[i+1]) / (2 n_valid (thr[T-1] - thr[0]))      (f64, rounded once)
// A point goes to the bin of its distance, the first i with thr[i] >= d (T: none), found by binary search in the f32 table itself; the bins are
// counted with integer LDS adds and a prefix sum over the bins gives hits.  No float atomics, fixed summation order: two launches give the same bits.
#include <algorithm>
#include "common.h"

namespace mhe { namespace pck {

constexpr int NT = 256;                              // threads of a workgroup: 4 waves
constexpr int PMAX = MHE_PCK_MAX_POINTS;             // 778
constexpr int TMAX = MHE_PCK_MAX_THRESHOLDS;         // 256
constexpr int HB = TMAX + 1;                         // bins of a histogram: one per threshold and the bin of the misses (odd: rows start on different banks)
constexpr int WG_TARGET = 2048;                      // workgroups asked for: 8 per CU on 256 CUs (as mesh_eval.hip)
// lanes that serve a hypothesis of at most that many points (16, 32 or 64; more points, up to 64: a wave).  Below 64, several hypotheses share a
// wave.  A build-time constant: tools/bench_pck_lanes.py builds the three forms side by side, and DESIGN.md has what it measured - at the
// joints' P = 21 two hypotheses per wave take 0.045 ms where one takes 0.068 ms (N = 2000, B = 64).
#ifndef MHE_PCK_SMALL_LANES
#define MHE_PCK_SMALL_LANES 32
#endif
constexpr int SMALL = MHE_PCK_SMALL_LANES;
static_assert(SMALL == 16 || SMALL == 32 || SMALL == 64, "MHE_PCK_SMALL_LANES is 16, 32 or 64");

template <int W>
__device__ __forceinline__ int group_sum_int(int v) {
#pragma unroll
    for (int o = W / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
template <int W>
__device__ __forceinline__ float group_sum(float v) {
#pragma unroll
    for (int o = W / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
template <int W>
__device__ __forceinline__ double group_sum(double v) {
#pragma unroll
    for (int o = W / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// the first i in [0, T) with th[i] >= d, T if there is none (a NaN d: T).  Every index read lies in [0, T) whatever the table holds.
__device__ __forceinline__ int bin_of(const float *th, int T, float d) {
    int lo = 0, n = T;
    while (n > 0) {
        const int half = n >> 1;
        if (th[lo + half] >= d) n = half;
        else { lo += half + 1; n -= half + 1; }
    }
    return lo;
}

// Workgroup (b, c): image b, hypotheses n0 .. n0 + g - 1.  The image's scaled target (x / y / z planes), its valid mask and the thresholds go to
// LDS once.  A group of L threads serves one hypothesis at a time, NT / L hypotheses in flight: L = 256 (the four waves, one histogram per wave,
// added when they are read) for P > 64, else a wave (or SMALL lanes for P <= SMALL, so that several hypotheses share a wave), each with a
// histogram of its own.  Thread gl of a group owns points gl, gl + L, ...; FL = min(L, 64) lanes finish a hypothesis: lane fl owns
// the C = ceil(T / FL) consecutive bins from fl C, a scan over the lanes turns bin counts into hits, and every bin is zeroed as it is read.
// Per round two barriers: the bins are counted | the bins are read and zero again.
template <int L>
__global__ __launch_bounds__(NT) void pck_kernel(const float *__restrict__ pred, const float *__restrict__ target, const float *__restrict__ scale,
                                                 const unsigned char *__restrict__ valid, const float *__restrict__ thr, int *__restrict__ hits,
                                                 float *__restrict__ auc, float *__restrict__ err, int N, int B, int P, int T, int G, int chunks,
                                                 float unit) {
    constexpr int FL = L < 64 ? L : 64, NG = NT / L, NH = NT / FL;
    __shared__ float tg[3][PMAX];
    __shared__ unsigned char vm[PMAX];
    __shared__ float th[TMAX];
    __shared__ int hist[NH][HB];
    __shared__ float red_e[NT / 64];
    __shared__ int red_n[NT / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.x / chunks, n0 = (blockIdx.x % chunks) * G;
    const int g = min(G, N - n0);
    const float su = scale[b] * unit;

    int cnt = 0;
    for (int v = tid; v < P; v += NT) {
        const float *t = target + ((size_t)b * P + v) * 3;
        tg[0][v] = t[0] * su; tg[1][v] = t[1] * su; tg[2][v] = t[2] * su;
        const unsigned char m = valid ? (valid[(size_t)b * P + v] != 0) : 1;
        vm[v] = m;
        cnt += m;
    }
    for (int i = tid; i < T; i += NT) th[i] = thr[i];
    for (int i = tid; i < NH * HB; i += NT) (&hist[0][0])[i] = 0;
    cnt = group_sum_int<64>(cnt);
    if (lane == 0) red_n[wave] = cnt;
    __syncthreads();
    const int nv = red_n[0] + red_n[1] + red_n[2] + red_n[3];

    const int grp = tid / L, gl = tid % L, fl = tid % FL;
    int *const h = hist[tid / FL];                  // L = 256: the wave's; else the group's
    const int C = (T + FL - 1) / FL, i0 = min(fl * C, T), i1 = min(i0 + C, T);
    const double span = (double)th[T - 1] - (double)th[0];
    for (int first = 0; first < g; first += NG) {
        const bool active = first + grp < g;
        const size_t r = (size_t)(n0 + first + grp) * B + b;
        float e = 0.f;
        if (active)
            for (int v = gl; v < P; v += L)
                if (vm[v]) {
                    const float *p = pred + (r * P + v) * 3;
                    const float dx = p[0] * su - tg[0][v], dy = p[1] * su - tg[1][v], dz = p[2] * su - tg[2][v];
                    const float d = sqrtf(fmaf(dz, dz, fmaf(dy, dy, dx * dx)));
                    e += d < __builtin_inff() ? d : __builtin_nanf("");          // a non-finite distance: err NaN, and bin T below
                    atomicAdd(&h[bin_of(th, T, d)], 1);
                }
        e = group_sum<FL>(e);
        if (L == NT && lane == 0) red_e[wave] = e;
        __syncthreads();                           // the bins are counted
        if (L < NT || wave == 0) {
            int s = 0;
            if (active)
                for (int i = i0; i < i1; ++i)
#pragma unroll
                    for (int w = 0; w < NH / NG; ++w) s += h[w * HB + i];
            int x = s;                             // inclusive scan over the FL lanes
#pragma unroll
            for (int o = 1; o < FL; o <<= 1) {
                const int t = __shfl_up(x, o, FL);
                if (fl >= o) x += t;
            }
            int run = x - s;                       // hits[i0 - 1]
            double a = 0.0;
            if (active) {
                for (int i = i0; i < i1; ++i) {
                    const int prev = run;
#pragma unroll
                    for (int w = 0; w < NH / NG; ++w) { run += h[w * HB + i]; h[w * HB + i] = 0; }
                    if (hits) hits[r * T + i] = run;
                    if (i > 0) a += ((double)th[i] - (double)th[i - 1]) * (double)(prev + run);
                }
                if (fl == 0)
#pragma unroll
                    for (int w = 0; w < NH / NG; ++w) h[w * HB + T] = 0;         // the misses
            }
            a = group_sum<FL>(a);
            if (active && fl == 0) {
                const float es = L == NT ? ((red_e[0] + red_e[1]) + red_e[2]) + red_e[3] : e;
                auc[r] = nv > 0 ? (float)(a / (2.0 * (double)nv * span)) : __builtin_nanf("");
                err[r] = nv > 0 ? es / (float)nv : __builtin_nanf("");
            }
        }
        __syncthreads();                           // the bins are zero again, red_e is read
    }
}

}}  // namespace mhe::pck

using namespace mhe;

extern "C" int mhe_pck_curve_f32(const float *pred, const float *target, const float *scale, const unsigned char *valid, const float *thr, float unit,
                                 int *hits, float *auc, float *err, int N, int B, int P, int T, void *stream) {
    MHE_REQUIRE(pred && target && scale && thr && auc && err, "mhe_pck_curve_f32: null pointer");
    MHE_REQUIRE(N > 0 && B > 0, "mhe_pck_curve_f32: N=%d B=%d", N, B);
    MHE_REQUIRE(P >= 1 && P <= pck::PMAX, "mhe_pck_curve_f32: P=%d (P in 1..%d)", P, pck::PMAX);
    MHE_REQUIRE(T >= 2 && T <= pck::TMAX, "mhe_pck_curve_f32: T=%d (T in 2..%d)", T, pck::TMAX);
    MHE_REQUIRE((long)N * B <= 0x7fffffffL, "mhe_pck_curve_f32: N*B=%ld rows (at most 2^31 - 1)", (long)N * B);
    MHE_REQUIRE(unit == unit, "mhe_pck_curve_f32: unit is NaN");
    MHE_REQUIRE(on_device(thr), "mhe_pck_curve_f32: thr must be device memory");
    const size_t R = (size_t)N * B;
    struct { const void *p; size_t n; } in[5] = {{pred, R * P * 12}, {target, (size_t)B * P * 12}, {scale, (size_t)B * 4}, {valid, (size_t)B * P},
                                                 {thr, (size_t)T * 4}},
                                        out[3] = {{hits, R * T * 4}, {auc, R * 4}, {err, R * 4}};
    for (int o = 0; o < 3; ++o) {
        for (int i = 0; i < 5; ++i) MHE_REQUIRE(disjoint(out[o].p, out[o].n, in[i].p, in[i].n), "mhe_pck_curve_f32: output %d overlaps input %d", o, i);
        for (int q = o + 1; q < 3; ++q) MHE_REQUIRE(disjoint(out[o].p, out[o].n, out[q].p, out[q].n), "mhe_pck_curve_f32: outputs %d and %d overlap", o, q);
    }
    // hypotheses per workgroup: as few as it takes to stay within WG_TARGET workgroups (mesh_eval.hip's rule) - more than one only when
    // N > ceil(WG_TARGET / B)
    int chunks = std::min(N, (pck::WG_TARGET + B - 1) / B);
    const int G = (N + chunks - 1) / chunks;
    chunks = (N + G - 1) / G;
    const dim3 grid((unsigned)((size_t)B * chunks));
#define MHE_LAUNCH(L)                                                                                                                              \
    hipLaunchKernelGGL(pck::pck_kernel<L>, grid, dim3(pck::NT), 0, (hipStream_t)stream, pred, target, scale, valid, thr, hits, auc, err, N, B, P, T, \
                       G, chunks, unit)
    if (P > 64) MHE_LAUNCH(256);
    else if (P > pck::SMALL) MHE_LAUNCH(64);
    else MHE_LAUNCH(pck::SMALL);
#undef MHE_LAUNCH
    return check_launch("pck_kernel");
}
