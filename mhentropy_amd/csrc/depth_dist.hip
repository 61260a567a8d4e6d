// Depth agreement of the hand mesh with the depth image and its reverse (criteria.depth_dist, ops.depth_dist / depth_dist_bwd):
// mhe_depth_dist_f32, mhe_depth_dist_bwd_f32.  The contract is the one written at the entries' declaration in include/mhe.h.
//   One workgroup per hypothesis (row r, image r % B).  The z-image in LDS holds a 64-bit word per sample: render.hip's order-preserving depth
//   key in the high half, the face index in the low half, EMPTY (all ones) where nothing covers.  Faces are thrown at it with a 64-bit LDS
//   atomicMin, so "nearest depth, lowest face among equal f32 depths" is the order of the words and does not depend on which face arrives
//   first.  Projection, face set-up and sample test are csrc/raster.h's, the ones mhe_render_mesh_f32 uses; faces with BIG samples or more in
//   their box go to the workgroup's list as there.  The observation image of the workgroup's image lies next to the z-image.
//   Resolve: thread t owns samples t, t + NT, ... in both passes (pass 1: |O|, |P| and the offset; pass 2: the residuals), every sum is f64,
//   added per thread in ascending sample order, then across the wave by a butterfly and across the waves in ascending order: fixed.
//   Reverse: the same front, then the weight g(p) of every sample replaces the observation in LDS; a thread takes faces t, t + NT, ... and
//   walks each face's clamped box in row-major order, keeping the samples the face won (low half of the word) and summing g(p) w_k(p) for its
//   three corners in f64 registers.  After a barrier the sums and the face's two slopes go to a table [F][5] that lies over the z-image and the
//   weights, which nobody reads any more; one thread per vertex then sums its incident (face, corner) entries in ascending order from the
//   host's vertex -> face table, and the camera gradient is the fixed-order workgroup sum over the vertices.  No atomics on floats, no workspace.
//   LDS: 32 KiB z-image + 16 KiB observation + 12 KiB projected vertices + 1.3 KiB lists and partials = 61.3 KiB for either kernel at any
//   shape within the limits: two workgroups (16 waves) per CU.
#include <cstddef>
#include "raster.h"

namespace mhe { namespace depth {

using raster::Band;
using raster::Camera;
using raster::Face;

constexpr int NT = 512, NW = NT / 64;      // threads and waves of a workgroup
constexpr int SMAX = MHE_DEPTH_MAX_SIZE, VMAX = MHE_DEPTH_MAX_VERTS, FMAX = MHE_DEPTH_MAX_FACES;
constexpr int BIG = 64, NBIG = 256;        // as render.hip: samples in the box from which a face goes to the workgroup's list; its length
constexpr int FPT = FMAX / NT;             // faces per thread in the reverse
constexpr int TW = 5;                      // words of a face's table entry: the sums of corners a, b, c, the slopes gx, gy
constexpr unsigned long long EMPTY = ~0ull;
typedef unsigned long long u64;

struct Shared {
    u64 z[SMAX * SMAX];                    // the z-image ...
    float w[SMAX * SMAX];                  // ... and right behind it the observation, later the weights: together the reverse's face table
    float sx[VMAX], sy[VMAX], sd[VMAX];
    int big[NBIG];
    double red[4][NW];
    int nbig, bad;
};
static_assert(sizeof(u64) * SMAX * SMAX + sizeof(float) * SMAX * SMAX >= sizeof(float) * TW * FMAX, "the face table lies over z and w");
static_assert(offsetof(Shared, w) == sizeof(u64) * SMAX * SMAX, "w follows z");
static_assert(FPT * NT == FMAX, "a thread's faces");

__device__ __forceinline__ bool fin(double x) { return fabs(x) < __builtin_inf(); }

// sums of up to four doubles over the workgroup, the same bits in every thread: butterfly in the wave, waves in ascending order
template <int K> __device__ __forceinline__ void block_sum(double (&v)[K], Shared &sh) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < K; ++k)
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v[k] += __shfl_xor(v[k], o, 64);
    __syncthreads();                       // the previous sum has been read
    if (lane == 0)
#pragma unroll
        for (int k = 0; k < K; ++k) sh.red[k][wave] = v[k];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) {
        double s = sh.red[k][0];
        for (int w = 1; w < NW; ++w) s += sh.red[k][w];
        v[k] = s;
    }
}

__device__ __forceinline__ void shade(const Face &f, int face, int x, int y, int S, u64 *z) {
    float d;
    if (raster::covers(f, x, y, d)) atomicMin(&z[y * S + x], ((u64)raster::key_of(d) << 32) | (unsigned)face);
}

struct Row {
    Camera cam;
    Band bd;
    const float *vr;
    double off, nO, nP;                    // the offset used; |O|, |P|
    bool bad;                              // a non-finite projected vertex, zscale or root_z: NaN and zero gradients
};

// one sample's residual: false outside P
__device__ __forceinline__ bool residual(const Shared &sh, int p, double off, double &e) {
    const float o = sh.w[p];
    const u64 word = sh.z[p];
    if (!(o > 0.f && o < __builtin_inff()) || word == EMPTY) return false;
    e = (double)raster::depth_of((unsigned)(word >> 32)) + off - (double)o;
    return true;
}

// projection, z-image, |O|, |P| and the offset of row r: what the forward and the reverse share
__device__ __forceinline__ void front(Shared &sh, Row &row, const float *__restrict__ verts, const int *__restrict__ faces,
                                      const float *__restrict__ logs_t, const float *__restrict__ zscale, const float *__restrict__ obs,
                                      const float *__restrict__ root_z, int B, int V, int F, int S) {
    const int tid = threadIdx.x;
    const size_t r = blockIdx.x, b = r % (size_t)B;
    Camera &cam = row.cam;
    cam.s = exp((double)logs_t[r * 3]); cam.tx = logs_t[r * 3 + 1]; cam.ty = logs_t[r * 3 + 2]; cam.half = 0.5 * S;
    cam.zs = zscale[b];
    row.bd.G = S; row.bd.y0 = 0; row.bd.y1 = S - 1;
    row.vr = verts + r * (size_t)V * 3;
    if (tid == 0) { sh.nbig = 0; sh.bad = !fin(cam.zs) || (root_z && !fin((double)root_z[b])); }
    __syncthreads();
    for (int v = tid; v < V; v += NT) {
        raster::project(row.vr + (size_t)v * 3, cam, sh.sx[v], sh.sy[v], sh.sd[v]);
        if (!(fin(sh.sx[v]) && fin(sh.sy[v]) && fin(sh.sd[v]))) sh.bad = 1;
    }
    const float *ob = obs + b * (size_t)S * S;
    for (int p = tid; p < S * S; p += NT) { sh.z[p] = EMPTY; sh.w[p] = ob[p]; }
    __syncthreads();
    row.bad = sh.bad != 0;
    row.off = 0.0; row.nO = 0.0; row.nP = 0.0;
    if (row.bad) return;
    Face f;
    for (int face = tid; face < F; face += NT) {
        if (!raster::setup(f, face, faces, row.vr, V, true, sh.sx, sh.sy, sh.sd, cam, row.bd)) continue;
        if ((f.x1 - f.x0 + 1) * (f.y1 - f.y0 + 1) >= BIG) {
            const int slot = atomicAdd(&sh.nbig, 1);
            if (slot < NBIG) { sh.big[slot] = face; continue; }           // (a full list: the thread does the face itself)
        }
        for (int y = f.y0; y <= f.y1; ++y)
            for (int x = f.x0; x <= f.x1; ++x) shade(f, face, x, y, S, sh.z);
    }
    __syncthreads();
    const int nb = min(sh.nbig, NBIG);
    for (int q = 0; q < nb; ++q) {
        const int face = sh.big[q];
        if (!raster::setup(f, face, faces, row.vr, V, true, sh.sx, sh.sy, sh.sd, cam, row.bd)) continue;      // (uniform)
        const int w = f.x1 - f.x0 + 1, n = w * (f.y1 - f.y0 + 1);
        for (int i = tid; i < n; i += NT) {
            const int yy = i / w;
            shade(f, face, f.x0 + i - yy * w, f.y0 + yy, S, sh.z);
        }
    }
    __syncthreads();
    double a[3] = {0.0, 0.0, 0.0};         // |O|, |P|, sum over P of obs - R
    for (int p = tid; p < S * S; p += NT) {
        const float o = sh.w[p];
        if (!(o > 0.f && o < __builtin_inff())) continue;
        a[0] += 1.0;
        const u64 word = sh.z[p];
        if (word == EMPTY) continue;
        a[1] += 1.0;
        a[2] += (double)o - (double)raster::depth_of((unsigned)(word >> 32));
    }
    block_sum(a, sh);
    row.nO = a[0]; row.nP = a[1];
    row.off = root_z ? (double)root_z[b] : (a[1] > 0.0 ? a[2] / a[1] : 0.0);
}

__global__ __launch_bounds__(NT) void depth_dist_kernel(const float *__restrict__ verts, const int *__restrict__ faces, const float *__restrict__ logs_t,
                                                        const float *__restrict__ zscale, const float *__restrict__ obs,
                                                        const float *__restrict__ root_z, float trunc, float *__restrict__ dist,
                                                        float *__restrict__ parts, int *__restrict__ face_img, float *__restrict__ resid_img, int B,
                                                        int V, int F, int S) {
    __shared__ Shared sh;
    const int tid = threadIdx.x;
    const size_t r = blockIdx.x;
    Row row;
    front(sh, row, verts, faces, logs_t, zscale, obs, root_z, B, V, F, S);
    const double tr = trunc;
    const float nan = __builtin_nanf("");
    double a[2] = {0.0, 0.0};              // sum over P of min(|e|, trunc); inliers
    for (int p = tid; p < S * S; p += NT) {
        double e;
        const bool in_p = !row.bad && residual(sh, p, row.off, e);
        if (in_p) {
            const bool in = fabs(e) < tr;
            a[0] += in ? fabs(e) : tr;
            a[1] += in ? 1.0 : 0.0;
        }
        if (face_img) face_img[r * S * S + p] = sh.z[p] == EMPTY ? -1 : (int)(unsigned)sh.z[p];
        if (resid_img) resid_img[r * S * S + p] = in_p ? (float)e : nan;
    }
    block_sum(a, sh);
    if (tid == 0) {
        const bool any = row.nO > 0.0;
        dist[r] = row.bad ? nan : any ? (float)((a[0] + tr * (row.nO - row.nP)) / row.nO) : 0.f;
        if (parts) {
            parts[r * 3] = row.bad ? nan : any ? (float)(row.nP / row.nO) : 0.f;
            parts[r * 3 + 1] = row.bad ? nan : (float)row.off;
            parts[r * 3 + 2] = row.bad ? nan : row.nP > 0.0 ? (float)(a[1] / row.nP) : 0.f;
        }
    }
}

__global__ __launch_bounds__(NT) void depth_dist_bwd_kernel(const float *__restrict__ verts, const int *__restrict__ faces, const float *__restrict__ logs_t,
                                                            const float *__restrict__ zscale, const float *__restrict__ obs,
                                                            const float *__restrict__ root_z, float trunc, const int *__restrict__ vf_start,
                                                            const int *__restrict__ vf_list, const float *__restrict__ g_dist,
                                                            float *__restrict__ g_verts, float *__restrict__ g_logs_t, int B, int V, int F, int S) {
    __shared__ Shared sh;
    const int tid = threadIdx.x;
    const size_t r = blockIdx.x;
    Row row;
    front(sh, row, verts, faces, logs_t, zscale, obs, root_z, B, V, F, S);
    float *gv = g_verts + r * (size_t)V * 3;
    if (row.bad || !(row.nP > 0.0)) {      // (uniform) nothing compared: zeros
        for (int i = tid; i < V * 3; i += NT) gv[i] = 0.f;
        if (tid < 3) g_logs_t[r * 3 + tid] = 0.f;
        return;
    }
    const double tr = trunc;
    // s(p) = sign(e) [|e| < trunc]; its sum over P is an integer
    double a[1] = {0.0};
    for (int p = tid; p < S * S; p += NT) {
        double e;
        if (residual(sh, p, row.off, e) && fabs(e) < tr) a[0] += e > 0.0 ? 1.0 : e < 0.0 ? -1.0 : 0.0;
    }
    block_sum(a, sh);
    const double ms = root_z ? 0.0 : a[0] / row.nP, k = (double)g_dist[r] / row.nO;
    for (int p = tid; p < S * S; p += NT) {                                // the weights take the observation's place (a thread's own samples)
        double e;
        float wgt = 0.f;
        if (residual(sh, p, row.off, e)) wgt = (float)(((fabs(e) < tr ? (e > 0.0 ? 1.0 : e < 0.0 ? -1.0 : 0.0) : 0.0) - ms) * k);
        sh.w[p] = wgt;
    }
    __syncthreads();
    float acc[FPT][TW];
#pragma unroll
    for (int it = 0; it < FPT; ++it) {
        const int face = tid + it * NT;
        double s0 = 0.0, s1 = 0.0, s2 = 0.0;
        Face f;
        f.gx = 0.0; f.gy = 0.0;
        if (face < F && raster::setup(f, face, faces, row.vr, V, true, sh.sx, sh.sy, sh.sd, row.cam, row.bd)) {
            for (int y = f.y0; y <= f.y1; ++y)
                for (int x = f.x0; x <= f.x1; ++x) {
                    const u64 word = sh.z[y * S + x];
                    if ((unsigned)word != (unsigned)face || word == EMPTY) continue;
                    const double wgt = sh.w[y * S + x];
                    if (wgt == 0.0) continue;
                    double w0, w1, w2;
                    raster::edges(f, x, y, w0, w1, w2);
                    const double q = wgt / (w0 + w1 + w2);                 // (the sample is inside: the sum is the doubled area, > 0)
                    s0 += q * w1; s1 += q * w2; s2 += q * w0;              // corners a, b, c
                }
        }
        acc[it][0] = (float)s0; acc[it][1] = (float)s1; acc[it][2] = (float)s2; acc[it][3] = (float)f.gx; acc[it][4] = (float)f.gy;
    }
    __syncthreads();                       // nobody reads the z-image or the weights any more
    float *table = reinterpret_cast<float *>(sh.z);
#pragma unroll
    for (int it = 0; it < FPT; ++it) {
        const int face = tid + it * NT;
        if (face < F)
#pragma unroll
            for (int j = 0; j < TW; ++j) table[face * TW + j] = acc[it][j];
    }
    __syncthreads();
    const double cs = row.cam.s * row.cam.half;                            // dX / dv_x
    double l[3] = {0.0, 0.0, 0.0};
    for (int v = tid; v < V; v += NT) {
        const int beg = min(max(vf_start[v], 0), 3 * F), end = min(max(vf_start[v + 1], beg), 3 * F);
        double gx = 0.0, gy = 0.0, gz = 0.0;
        for (int i = beg; i < end; ++i) {
            const int ent = vf_list[i], face = ent >> 2, c = ent & 3;
            if (ent < 0 || face >= F || c > 2) continue;                   // never used as an address
            const double A = table[face * TW + c];
            gx -= (double)table[face * TW + 3] * A;
            gy -= (double)table[face * TW + 4] * A;
            gz += A;
        }
        gv[v * 3] = (float)(gx * cs); gv[v * 3 + 1] = (float)(gy * cs); gv[v * 3 + 2] = (float)(gz * row.cam.zs);
        l[0] += (gx * (double)row.vr[v * 3] + gy * (double)row.vr[v * 3 + 1]) * cs;
        l[1] += gx * row.cam.half;
        l[2] += gy * row.cam.half;
    }
    block_sum(l, sh);
    if (tid < 3) g_logs_t[r * 3 + tid] = (float)l[tid];
}

}}  // namespace mhe::depth

using namespace mhe;

static int depth_args(const char *who, const void *verts, const void *faces, const void *logs_t, const void *zscale, const void *obs, float trunc, int N,
                      int B, int V, int F, int S) {
    MHE_REQUIRE(verts && faces && logs_t && zscale && obs, "%s: null pointer (verts, faces, logs_t, zscale, obs)", who);
    MHE_REQUIRE(N >= 1 && B >= 1 && (long long)N * B < (1ll << 31), "%s: N=%d B=%d (each >= 1, N B < 2^31)", who, N, B);
    MHE_REQUIRE(V >= 1 && V <= MHE_DEPTH_MAX_VERTS && F >= 1 && F <= MHE_DEPTH_MAX_FACES, "%s: V=%d F=%d (V in 1..%d, F in 1..%d)", who, V, F,
                MHE_DEPTH_MAX_VERTS, MHE_DEPTH_MAX_FACES);
    MHE_REQUIRE(S >= 1 && S <= MHE_DEPTH_MAX_SIZE, "%s: S=%d (S in 1..%d)", who, S, MHE_DEPTH_MAX_SIZE);
    MHE_REQUIRE(trunc > 0.f && trunc < __builtin_inff(), "%s: trunc=%g (positive and finite)", who, (double)trunc);
    return MHE_OK;
}

struct Range { const void *p; size_t n; };

static int depth_overlap(const char *who, const Range *in, int nin, const Range *out, int nout) {
    for (int o = 0; o < nout; ++o) {
        for (int i = 0; i < nin; ++i) MHE_REQUIRE(disjoint(out[o].p, out[o].n, in[i].p, in[i].n), "%s: output %d overlaps input %d", who, o, i);
        for (int q = 0; q < o; ++q) MHE_REQUIRE(disjoint(out[o].p, out[o].n, out[q].p, out[q].n), "%s: outputs %d and %d overlap", who, q, o);
    }
    return MHE_OK;
}

extern "C" int mhe_depth_dist_f32(const float *verts, const int *faces, const float *logs_t, const float *zscale, const float *obs, const float *root_z,
                                  float trunc, float *dist, float *parts, int *face_img, float *resid_img, int N, int B, int V, int F, int S,
                                  void *stream) {
    const char *who = "mhe_depth_dist_f32";
    if (int st = depth_args(who, verts, faces, logs_t, zscale, obs, trunc, N, B, V, F, S)) return st;
    MHE_REQUIRE(dist, "%s: null pointer (dist)", who);
    const size_t R = (size_t)N * B, img = (size_t)S * S * 4;
    const Range in[6] = {{verts, R * V * 12}, {faces, (size_t)F * 12}, {logs_t, R * 12}, {zscale, (size_t)B * 4}, {obs, (size_t)B * img}, {root_z, (size_t)B * 4}};
    const Range out[4] = {{dist, R * 4}, {parts, R * 12}, {face_img, R * img}, {resid_img, R * img}};
    if (int st = depth_overlap(who, in, 6, out, 4)) return st;
    hipLaunchKernelGGL(depth::depth_dist_kernel, dim3((unsigned)R), dim3(depth::NT), 0, (hipStream_t)stream, verts, faces, logs_t, zscale, obs, root_z, trunc,
                       dist, parts, face_img, resid_img, B, V, F, S);
    return check_launch("depth_dist_kernel");
}

extern "C" int mhe_depth_dist_bwd_f32(const float *verts, const int *faces, const float *logs_t, const float *zscale, const float *obs, const float *root_z,
                                      float trunc, const int *vf_start, const int *vf_list, const float *g_dist, float *g_verts, float *g_logs_t, int N,
                                      int B, int V, int F, int S, void *stream) {
    const char *who = "mhe_depth_dist_bwd_f32";
    if (int st = depth_args(who, verts, faces, logs_t, zscale, obs, trunc, N, B, V, F, S)) return st;
    MHE_REQUIRE(vf_start && vf_list && g_dist && g_verts && g_logs_t, "%s: null pointer (vf_start, vf_list, g_dist, g_verts, g_logs_t)", who);
    const size_t R = (size_t)N * B, img = (size_t)S * S * 4;
    const Range in[9] = {{verts, R * V * 12}, {faces, (size_t)F * 12}, {logs_t, R * 12}, {zscale, (size_t)B * 4}, {obs, (size_t)B * img},
                         {root_z, (size_t)B * 4}, {vf_start, (size_t)(V + 1) * 4}, {vf_list, (size_t)F * 12}, {g_dist, R * 4}};
    const Range out[2] = {{g_verts, R * V * 12}, {g_logs_t, R * 12}};
    if (int st = depth_overlap(who, in, 9, out, 2)) return st;
    hipLaunchKernelGGL(depth::depth_dist_bwd_kernel, dim3((unsigned)R), dim3(depth::NT), 0, (hipStream_t)stream, verts, faces, logs_t, zscale, obs, root_z,
                       trunc, vf_start, vf_list, g_dist, g_verts, g_logs_t, B, V, F, S);
    return check_launch("depth_dist_bwd_kernel");
}
