// Silhouette distance of the projected hand mesh to the image's hand mask, and its reverse (criteria.silhouette_dist, ops.silhouette_*).
//   p_v = exp(log s) v_xy + t;  pixel (i, j) of the S x S grid: centre c = ((2j+1)/S - 1, (2i+1)/S - 1), the square of half-width 1/S around it
//   inside = mean_v min_m box(p_v, c_m),  cover = mean_m min_v |c_m - p_v|,  dist = inside + cover,  m over the kept pixels M_b of the image
// The contract is written at the declarations in include/mhe.h.  f32 pair evaluations, squared distances compared and one square root per
// minimum, ties to the lowest index; every sum runs in a fixed order in f64 (a thread's own terms, the wave's butterfly, the four waves in
// order) and nothing is atomic: two launches give the same bits.  The pixel count never leaves the device.
// With an occluder (the _occ entries): O_b = the kept pixels of the occluder mask that are not in M_b, listed behind M_b in the same list
// (count = |M_b|, count_all = |M_b| + |O_b|).  inside takes its minimum over M_b u O_b - a vertex on the occluder costs 0 - and cover stays
// the mean over M_b alone: the occluder excuses vertices and attracts nothing.  |M_b| = 0 is the empty list whatever O_b holds.
#include "common.h"

namespace mhe { namespace silhouette {

constexpr int NT = 256, NW = NT / 64;                   // threads / waves of a workgroup
constexpr int SMAX = MHE_SILHOUETTE_MAX_SIZE, PMAX = SMAX * SMAX;
constexpr int VMAX = MHE_SILHOUETTE_MAX_VERTS;
constexpr int KV = (VMAX + NT - 1) / NT;                // vertices of one thread (v = k NT + tid)
constexpr int KM = 4, TM = NT * KM;                     // kept pixels of one thread; of one round of the cover direction
constexpr int KPIX = PMAX / NT;                         // grid pixels of one thread of the pixel-list kernel

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ float2 centre(int packed, float fS) {
    const int i = packed >> 16, j = packed & 0xffff;
    return make_float2((float)(2 * j + 1) / fS - 1.f, (float)(2 * i + 1) / fS - 1.f);
}

__device__ __forceinline__ float box_sq(float px, float py, const float2 &c, float h) {
    const float ax = fmaxf(fabsf(px - c.x) - h, 0.f), ay = fmaxf(fabsf(py - c.y) - h, 0.f);
    return fmaf(ay, ay, ax * ax);
}

// Mask -> kept pixels of image b = blockIdx.x in row-major order.  A thread owns `per` consecutive grid pixels, box-sums each in f64 (bytes
// count as 0 / 1) and keeps it when 2 sum >= k^2, i.e. mean >= 0.5; the workgroup's exclusive prefix sum of the threads' counts fixes where
// a thread's pixels go.  The list's tail is -1.
template <typename T>
__device__ __forceinline__ unsigned kept_bits(const T *img, int H, int S, int k, int p0, int p1) {
    const double half = 0.5 * (double)k * (double)k;
    unsigned keep = 0;
    for (int p = p0; p < p1; ++p) {
        const int i = p / S, j = p - i * S;
        double s = 0.0;
        for (int y = 0; y < k; ++y) {
            const T *row = img + (size_t)(i * k + y) * H + (size_t)j * k;
            for (int x = 0; x < k; ++x) s += sizeof(T) == 1 ? (row[x] != (T)0 ? 1.0 : 0.0) : (double)row[x];
        }
        if (s >= half) keep |= 1u << (p - p0);
    }
    return keep;
}

// inclusive prefix sum of `mine` over the wave's lanes
__device__ __forceinline__ int wave_incl(int mine, int lane) {
    int incl = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int up = __shfl_up(incl, o, 64);
        if (lane >= o) incl += up;
    }
    return incl;
}

// a thread's kept pixels to the list from position off on; returns the position behind them
__device__ __forceinline__ int put_pixels(int *out, int off, unsigned keep, int p0, int p1, int S) {
    for (int p = p0; p < p1; ++p)
        if (keep >> (p - p0) & 1u) {
            const int i = p / S;
            out[off++] = (i << 16) | (p - i * S);
        }
    return off;
}

template <typename T>
__global__ __launch_bounds__(NT) void pixels_kernel(const T *__restrict__ mask, int *__restrict__ pixels, int *__restrict__ count, int H, int S) {
    __shared__ int wtot[NW];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.x;
    const int P = S * S, per = (P + NT - 1) / NT, k = H / S;
    const int p0 = min(P, tid * per), p1 = min(P, p0 + per);
    const unsigned keep = kept_bits(mask + (size_t)b * H * H, H, S, k, p0, p1);
    const int mine = __popc(keep), incl = wave_incl(mine, lane);
    if (lane == 63) wtot[wave] = incl;
    __syncthreads();
    int off = incl - mine, total = 0;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
        if (w < wave) off += wtot[w];
        total += wtot[w];
    }
    int *out = pixels + (size_t)b * P;
    put_pixels(out, off, keep, p0, p1, S);
    for (int q = total + tid; q < P; q += NT) out[q] = -1;
    if (tid == 0) count[b] = total;
}

// The two-mask form: the hand's kept pixels M_b, then the occluder's that are not the hand's (O_b), then the -1 tail - two prefix sums, the
// occluder's offset by the hand total.  The sections are disjoint, so count_all <= S^2 and the list keeps its S^2 ints.
template <typename T, typename U>
__global__ __launch_bounds__(NT) void pixels_occ_kernel(const T *__restrict__ mask, const U *__restrict__ occ, int *__restrict__ pixels,
                                                        int *__restrict__ count, int *__restrict__ count_all, int H, int S) {
    __shared__ int wtot[2][NW];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.x;
    const int P = S * S, per = (P + NT - 1) / NT, k = H / S;
    const int p0 = min(P, tid * per), p1 = min(P, p0 + per);
    const unsigned keep = kept_bits(mask + (size_t)b * H * H, H, S, k, p0, p1);
    const unsigned okeep = kept_bits(occ + (size_t)b * H * H, H, S, k, p0, p1) & ~keep;
    const int mine = __popc(keep), omine = __popc(okeep), incl = wave_incl(mine, lane), oincl = wave_incl(omine, lane);
    if (lane == 63) { wtot[0][wave] = incl; wtot[1][wave] = oincl; }
    __syncthreads();
    int off = incl - mine, ooff = oincl - omine, total = 0, ototal = 0;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
        if (w < wave) { off += wtot[0][w]; ooff += wtot[1][w]; }
        total += wtot[0][w]; ototal += wtot[1][w];
    }
    int *out = pixels + (size_t)b * P;
    put_pixels(out, off, keep, p0, p1, S);
    put_pixels(out, total + ooff, okeep, p0, p1, S);
    for (int q = total + ototal + tid; q < P; q += NT) out[q] = -1;
    if (tid == 0) { count[b] = total; count_all[b] = total + ototal; }
}

// min over the image's M kept pixels (LDS, every lane reads the same centre: a broadcast) for K vertices held in registers
template <bool IDX, int K>
__device__ __forceinline__ void scan_pixels(const float2 *pc, int M, float h, const float *px, const float *py, float *m1, int *i1) {
#pragma unroll 4
    for (int m = 0; m < M; ++m) {
        const float2 c = pc[m];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const float d = box_sq(px[k], py[k], c, h);
            if (IDX) { if (d < m1[k]) { m1[k] = d; i1[k] = m; } }
            else m1[k] = fminf(m1[k], d);
        }
    }
}

// min over the row's V projected vertices (LDS, broadcast) for K kept pixels held in registers
template <bool IDX, int K>
__device__ __forceinline__ void scan_verts(const float2 *pv, int V, const float *cx, const float *cy, float *m2, int *i2) {
#pragma unroll
    for (int k = 0; k < K; ++k) { m2[k] = __builtin_inff(); i2[k] = 0; }
#pragma unroll 4
    for (int v = 0; v < V; ++v) {
        const float2 p = pv[v];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const float dx = cx[k] - p.x, dy = cy[k] - p.y, d = fmaf(dy, dy, dx * dx);
            if (IDX) { if (d < m2[k]) { m2[k] = d; i2[k] = v; } }
            else m2[k] = fminf(m2[k], d);
        }
    }
}

// u(p - c): the unit vector from centre c to the vertex at (qx, qy) the pixel chose; false (nothing to add) at distance 0
__device__ __forceinline__ bool cover_unit(float qx, float qy, const float2 &c, float &ux, float &uy) {
    const float dx = qx - c.x, dy = qy - c.y, q = fmaf(dy, dy, dx * dx);
    if (!(q > 0.f)) return false;
    const float inv = 1.f / sqrtf(q);
    ux = dx * inv; uy = dy * inv;
    return true;
}

// gradient of the box distance of the vertex at (qx, qy) to the pixel of centre c, 0 where the distance is 0
__device__ __forceinline__ void box_unit(float qx, float qy, const float2 &c, float h, float &ux, float &uy) {
    const float dx = qx - c.x, dy = qy - c.y;
    const float ax = fmaxf(fabsf(dx) - h, 0.f), ay = fmaxf(fabsf(dy) - h, 0.f), q = fmaf(ay, ay, ax * ax);
    ux = uy = 0.f;
    if (q > 0.f) {
        const float inv = 1.f / sqrtf(q);
        ux = copysignf(ax, dx) * inv; uy = copysignf(ay, dy) * inv;
    }
}

// The gather walk of the reverse: the thread that owns vertex v (tid = v mod NT, slot v / NT) walks the row's pixel -> vertex list in ascending
// m and adds the unit vectors of the pixels that chose v to its own registers.  vert_of(m): the listed vertex (an index outside 0 .. V-1
// contributes nothing and is never used as an address), centre_of(m): the pixel's centre.
struct ListGlobal {                // dist_bwd_kernel: idx_m and the packed pixels, staged in LDS
    const int *ti, *pk;
    float fS;
    __device__ __forceinline__ int vert_of(int m) const { return ti[m]; }
    __device__ __forceinline__ float2 centre_of(int m) const { return centre(pk[m], fS); }
};
struct ListLocal {                 // dist_grad_kernel: the 16-bit list and the decoded centres of its own forward
    const unsigned short *lv;
    const float2 *pc;
    __device__ __forceinline__ int vert_of(int m) const { return (int)lv[m]; }
    __device__ __forceinline__ float2 centre_of(int m) const { return pc[m]; }
};

template <typename List>
__device__ __forceinline__ void gather_walk(int M, int V, int tid, const float *px, const float *py, const List list, double *gx, double *gy) {
#pragma unroll
    for (int k = 0; k < KV; ++k) gx[k] = gy[k] = 0.0;
    for (int m = 0; m < M; ++m) {
        const int t = list.vert_of(m);
        if ((t & (NT - 1)) == tid && (unsigned)t < (unsigned)V) {
            const int slot = t / NT;
            float qx = px[0], qy = py[0];
#pragma unroll
            for (int k = 1; k < KV; ++k) { qx = slot == k ? px[k] : qx; qy = slot == k ? py[k] : qy; }
            float ux, uy;
            if (cover_unit(qx, qy, list.centre_of(m), ux, uy)) {
#pragma unroll
                for (int k = 0; k < KV; ++k) { gx[k] = slot == k ? gx[k] + (double)ux : gx[k]; gy[k] = slot == k ? gy[k] + (double)uy : gy[k]; }
            }
        }
    }
}

// g_p_v of one vertex from its two halves (u: the box gradient to its own pixel, (gx, gy): the walk's sum), its g_verts row and its terms of
// the three sums of g_logs_t
__device__ __forceinline__ void finish_vertex(float ux, float uy, double gx, double gy, double gd, double wV, double wM, float es, float vx, float vy,
                                              float *g, double &s_l, double &s_x, double &s_y) {
    const double gpx = gd * ((double)ux * wV + gx * wM), gpy = gd * ((double)uy * wV + gy * wM);
    g[0] = (float)((double)es * gpx); g[1] = (float)((double)es * gpy); g[2] = 0.f;
    s_l += gpx * (double)(es * vx) + gpy * (double)(es * vy);
    s_x += gpx; s_y += gpy;
}

// the row's (inside, cover) from the four waves' partial sums, in order; (0, 0) for an empty list
__device__ __forceinline__ float2 row_parts(const double (*red)[NW], int V, int M) {
    float I = 0.f, Cv = 0.f;
    if (M) {
        I = (float)((((red[0][0] + red[0][1]) + red[0][2]) + red[0][3]) / (double)V);
        Cv = (float)((((red[1][0] + red[1][1]) + red[1][2]) + red[1][3]) / (double)M);
    }
    return make_float2(I, Cv);
}

// The end of the image's list for the mesh -> mask scan: M (the hand section) without an occluder; with one, count_all clamped to M .. S^2 -
// and 0 with no hand pixel: such an image is the empty list whatever its occluder holds.
__device__ __forceinline__ int list_end(const int *count_all, int b, int M, int P) {
    return count_all && M ? min(max(count_all[b], M), P) : M;
}

// Forward, one workgroup per row r = n B + b.  The row's vertices are projected once (registers of their thread, and LDS for the cover
// direction), the image's kept pixels are decoded once into LDS as centres; both directional minima are taken from LDS.  The count is
// clamped to 0 .. S^2 before it bounds anything.  A non-finite projected vertex makes the row NaN (the flag, not the minima, carries it:
// fminf would drop the NaN); an empty list makes it 0.
template <bool IDX>
__global__ __launch_bounds__(NT) void dist_kernel(const float *__restrict__ verts, const float *__restrict__ logs_t, const int *__restrict__ pixels,
                                                  const int *__restrict__ count, const int *__restrict__ count_all, float *__restrict__ dist,
                                                  float *__restrict__ parts, int *__restrict__ idx_v, int *__restrict__ idx_m, int B, int V, int S) {
    __shared__ float2 pc[PMAX];
    __shared__ float2 pv[KV * NT];
    __shared__ double red[2][NW];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t r = blockIdx.x;
    const int b = (int)(r % (size_t)B), P = S * S, M = min(max(count[b], 0), P), M2 = list_end(count_all, b, M, P);
    const float fS = (float)S, h = 1.f / fS;
    const float es = expf(logs_t[r * 3]), tx = logs_t[r * 3 + 1], ty = logs_t[r * 3 + 2];

    float px[KV], py[KV], m1[KV];
    int i1[KV];
    int bad = 0;
#pragma unroll
    for (int k = 0; k < KV; ++k) {
        const int v = k * NT + tid;
        px[k] = py[k] = 0.f;
        m1[k] = __builtin_inff();
        i1[k] = 0;
        if (v < V) {
            const float *p = verts + (r * V + v) * 3;
            px[k] = fmaf(es, p[0], tx); py[k] = fmaf(es, p[1], ty);
            bad |= !(isfinite(px[k]) && isfinite(py[k]));
            pv[v] = make_float2(px[k], py[k]);
        }
    }
    for (int m = tid; m < M2; m += NT) pc[m] = centre(pixels[(size_t)b * P + m], fS);
    bad = __syncthreads_or(bad);

    // mesh -> mask
    switch ((V + NT - 1) / NT) {
#define MHE_CASE(K) case K: scan_pixels<IDX, K>(pc, M2, h, px, py, m1, i1); break;
        MHE_CASE(1) MHE_CASE(2) MHE_CASE(3) MHE_CASE(4)
#undef MHE_CASE
    }
    static_assert(KV == 4, "the switch above covers 1 .. KV vertices per thread");
    double s_in = 0.0, s_co = 0.0;
#pragma unroll
    for (int k = 0; k < KV; ++k) {
        const int v = k * NT + tid;
        if (v < V) {
            s_in += (double)sqrtf(m1[k]);
            if (IDX && idx_v) idx_v[r * V + v] = M ? i1[k] : -1;
        }
    }
    // mask -> mesh, rounds of TM kept pixels
    for (int t0 = 0; t0 < M; t0 += TM) {
        const int tm = min(TM, M - t0);
        float cx[KM], cy[KM], m2[KM];
        int i2[KM];
#pragma unroll
        for (int k = 0; k < KM; ++k) {
            const int m = k * NT + tid;
            const float2 c = m < tm ? pc[t0 + m] : make_float2(0.f, 0.f);
            cx[k] = c.x; cy[k] = c.y;
        }
        switch ((tm + NT - 1) / NT) {
#define MHE_CASE(K) case K: scan_verts<IDX, K>(pv, V, cx, cy, m2, i2); break;
            MHE_CASE(1) MHE_CASE(2) MHE_CASE(3) MHE_CASE(4)
#undef MHE_CASE
        }
        static_assert(KM == 4, "the switch above covers 1 .. KM pixels per thread");
#pragma unroll
        for (int k = 0; k < KM; ++k) {
            const int m = k * NT + tid;
            if (m < tm) {
                s_co += (double)sqrtf(m2[k]);
                if (IDX && idx_m) idx_m[r * P + t0 + m] = i2[k];
            }
        }
    }
    s_in = wave_sum(s_in); s_co = wave_sum(s_co);
    if (lane == 0) { red[0][wave] = s_in; red[1][wave] = s_co; }
    __syncthreads();
    if (tid == 0) {
        const float2 ic = row_parts(red, V, M);
        float I = ic.x, Cv = ic.y, D = I + Cv;
        if (bad) I = Cv = D = __builtin_nanf("");
        dist[r] = D;
        if (parts) { parts[r * 2] = I; parts[r * 2 + 1] = Cv; }
    }
    if (IDX && idx_m)
        for (int m = M + tid; m < P; m += NT) idx_m[r * P + m] = -1;
}

// Reverse, one workgroup per row.  The thread that owns vertex v (tid = v mod NT, slot v / NT) walks the row's pixel -> vertex list from LDS
// in ascending m and adds the unit vectors of the pixels that chose v to its own registers: a fixed order, nothing atomic.  An index outside
// its range contributes nothing and is never used as an address.  u(0) = 0.  A row with a non-finite projected vertex, or of an image with
// an empty list, gets zeros.
__global__ __launch_bounds__(NT) void dist_bwd_kernel(const float *__restrict__ verts, const float *__restrict__ logs_t, const int *__restrict__ pixels,
                                                      const int *__restrict__ count, const int *__restrict__ count_all,
                                                      const int *__restrict__ idx_v, const int *__restrict__ idx_m, const float *__restrict__ g_dist,
                                                      float *__restrict__ g_verts, float *__restrict__ g_logs_t, int B, int V, int S) {
    __shared__ int pk[PMAX];
    __shared__ int ti[PMAX];
    __shared__ double red[3][NW];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t r = blockIdx.x;
    const int b = (int)(r % (size_t)B), P = S * S, M = min(max(count[b], 0), P), M2 = list_end(count_all, b, M, P);
    const float fS = (float)S, h = 1.f / fS;
    const float es = expf(logs_t[r * 3]), tx = logs_t[r * 3 + 1], ty = logs_t[r * 3 + 2];

    float vx[KV], vy[KV], px[KV], py[KV];
    int bad = 0;
#pragma unroll
    for (int k = 0; k < KV; ++k) {
        const int v = k * NT + tid;
        vx[k] = vy[k] = px[k] = py[k] = 0.f;
        if (v < V) {
            const float *p = verts + (r * V + v) * 3;
            vx[k] = p[0]; vy[k] = p[1];
            px[k] = fmaf(es, vx[k], tx); py[k] = fmaf(es, vy[k], ty);
            bad |= !(isfinite(px[k]) && isfinite(py[k]));
        }
    }
    for (int m = tid; m < M2; m += NT) {
        pk[m] = pixels[(size_t)b * P + m];
        if (m < M) ti[m] = idx_m[r * P + m];
    }
    bad = __syncthreads_or(bad);
    if (bad || M == 0) {
#pragma unroll
        for (int k = 0; k < KV; ++k) {
            const int v = k * NT + tid;
            if (v < V) { float *g = g_verts + (r * V + v) * 3; g[0] = 0.f; g[1] = 0.f; g[2] = 0.f; }
        }
        if (tid < 3) g_logs_t[r * 3 + tid] = 0.f;
        return;
    }

    double gx[KV], gy[KV];
    gather_walk(M, V, tid, px, py, ListGlobal{ti, pk, fS}, gx, gy);

    const double gd = (double)g_dist[r], wV = 1.0 / (double)V, wM = 1.0 / (double)M;
    double s_l = 0.0, s_x = 0.0, s_y = 0.0;
#pragma unroll
    for (int k = 0; k < KV; ++k) {
        const int v = k * NT + tid;
        if (v < V) {
            float ux = 0.f, uy = 0.f;
            const int iv = idx_v[r * V + v];
            if ((unsigned)iv < (unsigned)M2) box_unit(px[k], py[k], centre(pk[iv], fS), h, ux, uy);
            finish_vertex(ux, uy, gx[k], gy[k], gd, wV, wM, es, vx[k], vy[k], g_verts + (r * V + v) * 3, s_l, s_x, s_y);
        }
    }
    s_l = wave_sum(s_l); s_x = wave_sum(s_x); s_y = wave_sum(s_y);
    if (lane == 0) { red[0][wave] = s_l; red[1][wave] = s_x; red[2][wave] = s_y; }
    __syncthreads();
    if (tid < 3) g_logs_t[r * 3 + tid] = (float)(((red[tid][0] + red[tid][1]) + red[tid][2]) + red[tid][3]);
}

// Forward and reverse of one row in one launch: what dist_kernel<true> followed by dist_bwd_kernel write, without the two index tensors.  The
// vertex's own (min, argmin pixel) stays in the registers of its owner; every kept pixel's argmin vertex (V <= 778: 16 bits) goes to an LDS
// list in the rounds of the forward, and after the barrier the owners walk that list as dist_bwd_kernel walks idx_m.  The centres the walk
// needs are the decoded ones of the forward.  dist may be null.
__global__ __launch_bounds__(NT) void dist_grad_kernel(const float *__restrict__ verts, const float *__restrict__ logs_t, const int *__restrict__ pixels,
                                                       const int *__restrict__ count, const int *__restrict__ count_all,
                                                       const float *__restrict__ g_dist, float *__restrict__ dist, float *__restrict__ g_verts,
                                                       float *__restrict__ g_logs_t, int B, int V, int S) {
    __shared__ float2 pc[PMAX];
    __shared__ float2 pv[KV * NT];
    __shared__ unsigned short lv[PMAX];
    __shared__ double red[2][NW];
    __shared__ double red3[3][NW];
    static_assert(VMAX <= 0xffff, "a listed vertex is 16 bits");
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t r = blockIdx.x;
    const int b = (int)(r % (size_t)B), P = S * S, M = min(max(count[b], 0), P), M2 = list_end(count_all, b, M, P);
    const float fS = (float)S, h = 1.f / fS;
    const float es = expf(logs_t[r * 3]), tx = logs_t[r * 3 + 1], ty = logs_t[r * 3 + 2];

    float vx[KV], vy[KV], px[KV], py[KV], m1[KV];
    int i1[KV];
    int bad = 0;
#pragma unroll
    for (int k = 0; k < KV; ++k) {
        const int v = k * NT + tid;
        vx[k] = vy[k] = px[k] = py[k] = 0.f;
        m1[k] = __builtin_inff();
        i1[k] = 0;
        if (v < V) {
            const float *p = verts + (r * V + v) * 3;
            vx[k] = p[0]; vy[k] = p[1];
            px[k] = fmaf(es, vx[k], tx); py[k] = fmaf(es, vy[k], ty);
            bad |= !(isfinite(px[k]) && isfinite(py[k]));
            pv[v] = make_float2(px[k], py[k]);
        }
    }
    for (int m = tid; m < M2; m += NT) pc[m] = centre(pixels[(size_t)b * P + m], fS);
    bad = __syncthreads_or(bad);
    if (bad || M == 0) {
#pragma unroll
        for (int k = 0; k < KV; ++k) {
            const int v = k * NT + tid;
            if (v < V) { float *g = g_verts + (r * V + v) * 3; g[0] = 0.f; g[1] = 0.f; g[2] = 0.f; }
        }
        if (tid < 3) g_logs_t[r * 3 + tid] = 0.f;
        if (tid == 0 && dist) dist[r] = bad ? __builtin_nanf("") : 0.f;
        return;
    }

    // mesh -> mask: (min, argmin) of the thread's own vertices
    switch ((V + NT - 1) / NT) {
#define MHE_CASE(K) case K: scan_pixels<true, K>(pc, M2, h, px, py, m1, i1); break;
        MHE_CASE(1) MHE_CASE(2) MHE_CASE(3) MHE_CASE(4)
#undef MHE_CASE
    }
    double s_in = 0.0, s_co = 0.0;
#pragma unroll
    for (int k = 0; k < KV; ++k)
        if (k * NT + tid < V) s_in += (double)sqrtf(m1[k]);
    // mask -> mesh, rounds of TM kept pixels: the argmin vertex of pixel m to the LDS list
    for (int t0 = 0; t0 < M; t0 += TM) {
        const int tm = min(TM, M - t0);
        float cx[KM], cy[KM], m2[KM];
        int i2[KM];
#pragma unroll
        for (int k = 0; k < KM; ++k) {
            const int m = k * NT + tid;
            const float2 c = m < tm ? pc[t0 + m] : make_float2(0.f, 0.f);
            cx[k] = c.x; cy[k] = c.y;
        }
        switch ((tm + NT - 1) / NT) {
#define MHE_CASE(K) case K: scan_verts<true, K>(pv, V, cx, cy, m2, i2); break;
            MHE_CASE(1) MHE_CASE(2) MHE_CASE(3) MHE_CASE(4)
#undef MHE_CASE
        }
#pragma unroll
        for (int k = 0; k < KM; ++k) {
            const int m = k * NT + tid;
            if (m < tm) {
                s_co += (double)sqrtf(m2[k]);
                lv[t0 + m] = (unsigned short)i2[k];
            }
        }
    }
    s_in = wave_sum(s_in); s_co = wave_sum(s_co);
    if (lane == 0) { red[0][wave] = s_in; red[1][wave] = s_co; }
    __syncthreads();                       // the sums and the list
    if (tid == 0 && dist) {
        const float2 ic = row_parts(red, V, M);
        dist[r] = ic.x + ic.y;
    }

    double gx[KV], gy[KV];
    gather_walk(M, V, tid, px, py, ListLocal{lv, pc}, gx, gy);

    const double gd = (double)g_dist[r], wV = 1.0 / (double)V, wM = 1.0 / (double)M;
    double s_l = 0.0, s_x = 0.0, s_y = 0.0;
#pragma unroll
    for (int k = 0; k < KV; ++k) {
        const int v = k * NT + tid;
        if (v < V) {
            float ux, uy;
            box_unit(px[k], py[k], pc[i1[k]], h, ux, uy);
            finish_vertex(ux, uy, gx[k], gy[k], gd, wV, wM, es, vx[k], vy[k], g_verts + (r * V + v) * 3, s_l, s_x, s_y);
        }
    }
    s_l = wave_sum(s_l); s_x = wave_sum(s_x); s_y = wave_sum(s_y);
    if (lane == 0) { red3[0][wave] = s_l; red3[1][wave] = s_x; red3[2][wave] = s_y; }
    __syncthreads();
    if (tid < 3) g_logs_t[r * 3 + tid] = (float)(((red3[tid][0] + red3[tid][1]) + red3[tid][2]) + red3[tid][3]);
}

}}  // namespace mhe::silhouette

using namespace mhe;

// the shared argument checks of the forward and the reverse; R = N B rows
static int silhouette_args(const char *who, const void *verts, const void *logs_t, const void *pixels, const void *count, int N, int B, int V, int S) {
    MHE_REQUIRE(verts && logs_t && pixels && count, "%s: null pointer", who);
    MHE_REQUIRE(N > 0 && B > 0, "%s: N=%d B=%d", who, N, B);
    MHE_REQUIRE(V >= 1 && V <= silhouette::VMAX, "%s: V=%d (V in 1..%d)", who, V, silhouette::VMAX);
    MHE_REQUIRE(S >= 1 && S <= silhouette::SMAX, "%s: S=%d (S in 1..%d)", who, S, silhouette::SMAX);
    MHE_REQUIRE((long)N * B <= 0x7fffffffL, "%s: N*B=%ld rows (at most 2^31 - 1)", who, (long)N * B);
    return MHE_OK;
}

extern "C" int mhe_silhouette_pixels(const void *mask, int mask_is_float, int *pixels, int *count, int B, int H, int S, void *stream) {
    MHE_REQUIRE(mask && pixels && count, "mhe_silhouette_pixels: null pointer");
    MHE_REQUIRE(mask_is_float == 0 || mask_is_float == 1, "mhe_silhouette_pixels: mask_is_float=%d (0: bytes, 1: f32)", mask_is_float);
    MHE_REQUIRE(B > 0, "mhe_silhouette_pixels: B=%d", B);
    MHE_REQUIRE(S >= 1 && S <= silhouette::SMAX, "mhe_silhouette_pixels: S=%d (S in 1..%d)", S, silhouette::SMAX);
    MHE_REQUIRE(H >= S && H % S == 0 && H <= MHE_SILHOUETTE_MAX_MASK, "mhe_silhouette_pixels: H=%d (a multiple of S=%d, at most %d)", H, S,
                MHE_SILHOUETTE_MAX_MASK);
    const size_t nm = (size_t)B * H * H * (mask_is_float ? 4 : 1), np = (size_t)B * S * S * 4, nc = (size_t)B * 4;
    MHE_REQUIRE(disjoint(pixels, np, mask, nm) && disjoint(count, nc, mask, nm) && disjoint(pixels, np, count, nc),
                "mhe_silhouette_pixels: pixels, count and mask overlap");
    static_assert(silhouette::KPIX <= 32, "a thread's kept pixels are one 32-bit word");
    if (mask_is_float)
        hipLaunchKernelGGL(silhouette::pixels_kernel<float>, dim3((unsigned)B), dim3(silhouette::NT), 0, (hipStream_t)stream, (const float *)mask, pixels,
                           count, H, S);
    else
        hipLaunchKernelGGL(silhouette::pixels_kernel<unsigned char>, dim3((unsigned)B), dim3(silhouette::NT), 0, (hipStream_t)stream,
                           (const unsigned char *)mask, pixels, count, H, S);
    return check_launch("silhouette::pixels_kernel");
}

template <typename T>
static void launch_pixels_occ(const T *mask, const void *occ, int occ_is_float, int *pixels, int *count, int *count_all, int B, int H, int S, void *stream) {
    if (occ_is_float)
        hipLaunchKernelGGL((silhouette::pixels_occ_kernel<T, float>), dim3((unsigned)B), dim3(silhouette::NT), 0, (hipStream_t)stream, mask,
                           (const float *)occ, pixels, count, count_all, H, S);
    else
        hipLaunchKernelGGL((silhouette::pixels_occ_kernel<T, unsigned char>), dim3((unsigned)B), dim3(silhouette::NT), 0, (hipStream_t)stream, mask,
                           (const unsigned char *)occ, pixels, count, count_all, H, S);
}

extern "C" int mhe_silhouette_pixels_occ(const void *mask, int mask_is_float, const void *occluder, int occluder_is_float, int *pixels, int *count,
                                         int *count_all, int B, int H, int S, void *stream) {
    MHE_REQUIRE(mask && occluder && pixels && count && count_all, "mhe_silhouette_pixels_occ: null pointer");
    MHE_REQUIRE((mask_is_float == 0 || mask_is_float == 1) && (occluder_is_float == 0 || occluder_is_float == 1),
                "mhe_silhouette_pixels_occ: mask_is_float=%d occluder_is_float=%d (0: bytes, 1: f32)", mask_is_float, occluder_is_float);
    MHE_REQUIRE(B > 0, "mhe_silhouette_pixels_occ: B=%d", B);
    MHE_REQUIRE(S >= 1 && S <= silhouette::SMAX, "mhe_silhouette_pixels_occ: S=%d (S in 1..%d)", S, silhouette::SMAX);
    MHE_REQUIRE(H >= S && H % S == 0 && H <= MHE_SILHOUETTE_MAX_MASK, "mhe_silhouette_pixels_occ: H=%d (a multiple of S=%d, at most %d)", H, S,
                MHE_SILHOUETTE_MAX_MASK);
    const size_t px = (size_t)B * H * H, nc = (size_t)B * 4;
    struct { const void *p; size_t n; } in[2] = {{mask, px * (mask_is_float ? 4 : 1)}, {occluder, px * (occluder_is_float ? 4 : 1)}},
                                        out[3] = {{pixels, (size_t)B * S * S * 4}, {count, nc}, {count_all, nc}};
    for (int o = 0; o < 3; ++o) {
        for (int i = 0; i < 2; ++i)
            MHE_REQUIRE(disjoint(out[o].p, out[o].n, in[i].p, in[i].n), "mhe_silhouette_pixels_occ: output %d overlaps input %d", o, i);
        for (int q = 0; q < o; ++q)
            MHE_REQUIRE(disjoint(out[o].p, out[o].n, out[q].p, out[q].n), "mhe_silhouette_pixels_occ: outputs %d and %d overlap", q, o);
    }
    if (mask_is_float)
        launch_pixels_occ((const float *)mask, occluder, occluder_is_float, pixels, count, count_all, B, H, S, stream);
    else
        launch_pixels_occ((const unsigned char *)mask, occluder, occluder_is_float, pixels, count, count_all, B, H, S, stream);
    return check_launch("silhouette::pixels_occ_kernel");
}

// The three distance entries and their _occ forms share their bodies: count_all is null for the former (occ = false) and required for the latter.
static int dist_call(const char *who, bool occ, const float *verts, const float *logs_t, const int *pixels, const int *count, const int *count_all,
                     float *dist, float *parts, int *idx_v, int *idx_m, int N, int B, int V, int S, void *stream) {
    if (int st = silhouette_args(who, verts, logs_t, pixels, count, N, B, V, S)) return st;
    MHE_REQUIRE(dist, "%s: null pointer (dist)", who);
    MHE_REQUIRE(!occ || count_all, "%s: null pointer (count_all)", who);
    const size_t R = (size_t)N * B, P = (size_t)S * S;
    struct { const void *p; size_t n; } in[5] = {{verts, R * V * 12}, {logs_t, R * 12}, {pixels, (size_t)B * P * 4}, {count, (size_t)B * 4},
                                                 {count_all, (size_t)B * 4}},
                                        out[4] = {{dist, R * 4}, {parts, R * 8}, {idx_v, R * V * 4}, {idx_m, R * P * 4}};
    for (int o = 0; o < 4; ++o) {
        for (int i = 0; i < 5; ++i)
            MHE_REQUIRE(disjoint(out[o].p, out[o].n, in[i].p, in[i].n), "%s: output %d overlaps input %d", who, o, i);
        for (int q = 0; q < o; ++q)
            MHE_REQUIRE(disjoint(out[o].p, out[o].n, out[q].p, out[q].n), "%s: outputs %d and %d overlap", who, q, o);
    }
    if (idx_v || idx_m)
        hipLaunchKernelGGL(silhouette::dist_kernel<true>, dim3((unsigned)R), dim3(silhouette::NT), 0, (hipStream_t)stream, verts, logs_t, pixels, count,
                           count_all, dist, parts, idx_v, idx_m, B, V, S);
    else
        hipLaunchKernelGGL(silhouette::dist_kernel<false>, dim3((unsigned)R), dim3(silhouette::NT), 0, (hipStream_t)stream, verts, logs_t, pixels, count,
                           count_all, dist, parts, idx_v, idx_m, B, V, S);
    return check_launch("silhouette::dist_kernel");
}

static int dist_bwd_call(const char *who, bool occ, const float *verts, const float *logs_t, const int *pixels, const int *count, const int *count_all,
                         const int *idx_v, const int *idx_m, const float *g_dist, float *g_verts, float *g_logs_t, int N, int B, int V, int S,
                         void *stream) {
    if (int st = silhouette_args(who, verts, logs_t, pixels, count, N, B, V, S)) return st;
    MHE_REQUIRE(idx_v && idx_m && g_dist && g_verts && g_logs_t, "%s: null pointer (idx_v, idx_m, g_dist, g_verts, g_logs_t)", who);
    MHE_REQUIRE(!occ || count_all, "%s: null pointer (count_all)", who);
    const size_t R = (size_t)N * B, P = (size_t)S * S;
    struct { const void *p; size_t n; } in[8] = {{verts, R * V * 12}, {logs_t, R * 12}, {pixels, (size_t)B * P * 4}, {count, (size_t)B * 4},
                                                 {idx_v, R * V * 4}, {idx_m, R * P * 4}, {g_dist, R * 4}, {count_all, (size_t)B * 4}};
    for (int i = 0; i < 8; ++i)
        MHE_REQUIRE(disjoint(g_verts, R * V * 12, in[i].p, in[i].n) && disjoint(g_logs_t, R * 12, in[i].p, in[i].n), "%s: an output overlaps input %d",
                    who, i);
    MHE_REQUIRE(disjoint(g_verts, R * V * 12, g_logs_t, R * 12), "%s: g_verts and g_logs_t overlap", who);
    hipLaunchKernelGGL(silhouette::dist_bwd_kernel, dim3((unsigned)R), dim3(silhouette::NT), 0, (hipStream_t)stream, verts, logs_t, pixels, count, count_all,
                       idx_v, idx_m, g_dist, g_verts, g_logs_t, B, V, S);
    return check_launch("silhouette::dist_bwd_kernel");
}

static int dist_grad_call(const char *who, bool occ, const float *verts, const float *logs_t, const int *pixels, const int *count, const int *count_all,
                          const float *g_dist, float *dist, float *g_verts, float *g_logs_t, int N, int B, int V, int S, void *stream) {
    if (int st = silhouette_args(who, verts, logs_t, pixels, count, N, B, V, S)) return st;
    MHE_REQUIRE(g_dist && g_verts && g_logs_t, "%s: null pointer (g_dist, g_verts, g_logs_t)", who);
    MHE_REQUIRE(!occ || count_all, "%s: null pointer (count_all)", who);
    const size_t R = (size_t)N * B, P = (size_t)S * S;
    struct { const void *p; size_t n; } in[6] = {{verts, R * V * 12}, {logs_t, R * 12}, {pixels, (size_t)B * P * 4}, {count, (size_t)B * 4}, {g_dist, R * 4},
                                                 {count_all, (size_t)B * 4}},
                                        out[3] = {{dist, R * 4}, {g_verts, R * V * 12}, {g_logs_t, R * 12}};
    for (int o = 0; o < 3; ++o) {
        for (int i = 0; i < 6; ++i)
            MHE_REQUIRE(disjoint(out[o].p, out[o].n, in[i].p, in[i].n), "%s: output %d overlaps input %d", who, o, i);
        for (int q = 0; q < o; ++q)
            MHE_REQUIRE(disjoint(out[o].p, out[o].n, out[q].p, out[q].n), "%s: outputs %d and %d overlap", who, q, o);
    }
    hipLaunchKernelGGL(silhouette::dist_grad_kernel, dim3((unsigned)R), dim3(silhouette::NT), 0, (hipStream_t)stream, verts, logs_t, pixels, count, count_all,
                       g_dist, dist, g_verts, g_logs_t, B, V, S);
    return check_launch("silhouette::dist_grad_kernel");
}

extern "C" int mhe_silhouette_dist_f32(const float *verts, const float *logs_t, const int *pixels, const int *count, float *dist, float *parts, int *idx_v,
                                       int *idx_m, int N, int B, int V, int S, void *stream) {
    return dist_call("mhe_silhouette_dist_f32", false, verts, logs_t, pixels, count, nullptr, dist, parts, idx_v, idx_m, N, B, V, S, stream);
}

extern "C" int mhe_silhouette_dist_occ_f32(const float *verts, const float *logs_t, const int *pixels, const int *count, const int *count_all, float *dist,
                                           float *parts, int *idx_v, int *idx_m, int N, int B, int V, int S, void *stream) {
    return dist_call("mhe_silhouette_dist_occ_f32", true, verts, logs_t, pixels, count, count_all, dist, parts, idx_v, idx_m, N, B, V, S, stream);
}

extern "C" int mhe_silhouette_dist_bwd_f32(const float *verts, const float *logs_t, const int *pixels, const int *count, const int *idx_v, const int *idx_m,
                                           const float *g_dist, float *g_verts, float *g_logs_t, int N, int B, int V, int S, void *stream) {
    return dist_bwd_call("mhe_silhouette_dist_bwd_f32", false, verts, logs_t, pixels, count, nullptr, idx_v, idx_m, g_dist, g_verts, g_logs_t, N, B, V, S,
                         stream);
}

extern "C" int mhe_silhouette_dist_bwd_occ_f32(const float *verts, const float *logs_t, const int *pixels, const int *count, const int *count_all,
                                               const int *idx_v, const int *idx_m, const float *g_dist, float *g_verts, float *g_logs_t, int N, int B, int V,
                                               int S, void *stream) {
    return dist_bwd_call("mhe_silhouette_dist_bwd_occ_f32", true, verts, logs_t, pixels, count, count_all, idx_v, idx_m, g_dist, g_verts, g_logs_t, N, B, V,
                         S, stream);
}

extern "C" int mhe_silhouette_dist_grad_f32(const float *verts, const float *logs_t, const int *pixels, const int *count, const float *g_dist, float *dist,
                                            float *g_verts, float *g_logs_t, int N, int B, int V, int S, void *stream) {
    return dist_grad_call("mhe_silhouette_dist_grad_f32", false, verts, logs_t, pixels, count, nullptr, g_dist, dist, g_verts, g_logs_t, N, B, V, S, stream);
}

extern "C" int mhe_silhouette_dist_grad_occ_f32(const float *verts, const float *logs_t, const int *pixels, const int *count, const int *count_all,
                                                const float *g_dist, float *dist, float *g_verts, float *g_logs_t, int N, int B, int V, int S,
                                                void *stream) {
    return dist_grad_call("mhe_silhouette_dist_grad_occ_f32", true, verts, logs_t, pixels, count, count_all, g_dist, dist, g_verts, g_logs_t, N, B, V, S,
                          stream);
}
