// Silhouette and depth of a triangle mesh under the orthographic camera of the 2D head (ManoLayer.render, ops.render_mesh,
// criteria.silhouette_iou): mhe_render_mesh_f32.  The contract is the one written at the entry's declaration in include/mhe.h.
//   One workgroup renders one row band of one hypothesis into a depth image in LDS: a word per sample holds the order-preserving integer
//   image of the nearest depth (EMPTY where nothing covers), faces are thrown at it with atomicMin - coverage and depth do not depend on the
//   order in which faces arrive.  A thread takes a face: bounding box clamped to the band, every sample of the box tested.  A face whose box
//   holds BIG samples or more is put on a list and rasterised by the whole workgroup afterwards (a face that covers the image would
//   otherwise keep one thread busy for 16k samples).  The pixels are then resolved from LDS: mask = covered samples / A^2, depth = nearest
//   covered sample, and min / max against the target summed in a fixed order - the mask need not be written at all.
//   The projection, the face set-up and the sample test are csrc/raster.h's (shared with csrc/depth_dist.hip); their arithmetic is noted there.
#include <algorithm>
#include "raster.h"

namespace mhe { namespace render {

constexpr int NT = 512;                    // threads of a workgroup
constexpr int ZW = 16384;                  // depth words of one band (64 KiB): a 64 x 64 anti-aliased image whole
constexpr int VS = 1024;                   // vertices staged in LDS (12 KiB); a larger mesh projects its vertices per face from global memory
constexpr int BIG = 64, NBIG = 256;        // samples in the clamped box from which a face goes to the workgroup's list; its length
constexpr unsigned EMPTY = 0xffffffffu;    // above the image of every number (+inf is 0xff800000)
// two workgroups per CU: 2 (64 + 12 + 1 KiB and a few words) < 160 KiB

using raster::Band;
using raster::Camera;
using raster::Face;
using raster::depth_of;
using raster::key_of;
using raster::project;
using raster::setup;

// sample (x, y) of the band against one face; x in [0, G), y in [band.y0, band.y1]
__device__ __forceinline__ void shade(const Face &f, int x, int y, const Band &bd, unsigned *zbuf) {
    float d;
    if (raster::covers(f, x, y, d)) atomicMin(&zbuf[(y - bd.y0) * bd.G + x], key_of(d));
}

// Workgroup (r, y): hypothesis r, bands y, y + gridDim.y, ...  - gridDim.y is the band count for an image-only call and 1 when a score is
// asked for: a score is summed by ONE workgroup over its row's bands in ascending order, which needs no workspace and fixes the order.
__global__ __launch_bounds__(NT) void render_kernel(const float *__restrict__ verts, const int *__restrict__ faces, const float *__restrict__ scale,
                                                    const float *__restrict__ trans, const float *__restrict__ zscale, const float *__restrict__ target,
                                                    float *__restrict__ mask, float *__restrict__ depth, float *__restrict__ iou_sums, int B, int V, int F,
                                                    int S, int A, int BR, int nbands, float far) {
    __shared__ unsigned zbuf[ZW];
    __shared__ float sx[VS], sy[VS], sd[VS];
    __shared__ int big[NBIG];
    __shared__ int nbig;
    __shared__ float part[2][NT / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t r = blockIdx.x;
    const int G = S * A;
    Camera cam;
    cam.s = fabs((double)scale[r]); cam.tx = trans[r * 2]; cam.ty = trans[r * 2 + 1]; cam.half = 0.5 * G;
    cam.zs = zscale ? (double)zscale[r] * 1e-3 : 1.0;
    const float *vr = verts + r * (size_t)V * 3;
    const bool staged = V <= VS;
    if (staged)
        for (int v = tid; v < V; v += NT) project(vr + (size_t)v * 3, cam, sx[v], sy[v], sd[v]);
    const float *tg = target ? target + (r % (size_t)B) * S * S : nullptr;
    const float inv_a2 = 1.f / (float)(A * A);
    float inter = 0.f, uni = 0.f;

    for (int band = blockIdx.y; band < nbands; band += gridDim.y) {
        Band bd;
        bd.G = G; bd.y0 = band * BR; bd.y1 = min(bd.y0 + BR, G) - 1;
        const int words = (bd.y1 - bd.y0 + 1) * G;         // <= ZW
        __syncthreads();                                   // the previous band is resolved (first pass: the vertex stage is written)
        for (int i = tid; i < words; i += NT) zbuf[i] = EMPTY;
        if (tid == 0) nbig = 0;
        __syncthreads();
        Face f;
        for (int face = tid; face < F; face += NT) {
            if (!setup(f, face, faces, vr, V, staged, sx, sy, sd, cam, bd)) continue;
            if ((f.x1 - f.x0 + 1) * (f.y1 - f.y0 + 1) >= BIG) {
                const int slot = atomicAdd(&nbig, 1);
                if (slot < NBIG) { big[slot] = face; continue; }           // (a full list: the thread does the face itself)
            }
            for (int y = f.y0; y <= f.y1; ++y)
                for (int x = f.x0; x <= f.x1; ++x) shade(f, x, y, bd, zbuf);
        }
        __syncthreads();
        const int nb = min(nbig, NBIG);
        for (int q = 0; q < nb; ++q) {
            if (!setup(f, big[q], faces, vr, V, staged, sx, sy, sd, cam, bd)) continue;      // (uniform: every thread sets up the same face)
            const int w = f.x1 - f.x0 + 1, n = w * (f.y1 - f.y0 + 1);
            for (int i = tid; i < n; i += NT) {
                const int yy = i / w;
                shade(f, f.x0 + i - yy * w, f.y0 + yy, bd, zbuf);
            }
        }
        __syncthreads();
        // resolve the band's pixels; thread t takes pixels t, t + NT, ... - its two sums grow in that order, band after band
        const int prow0 = bd.y0 / A, npix = (bd.y1 - bd.y0 + 1) / A * S;
        for (int p = tid; p < npix; p += NT) {
            const int pi = p / S, pj = p - pi * S;
            unsigned kmin = EMPTY;
            int cnt = 0;
            for (int a = 0; a < A; ++a)
                for (int b = 0; b < A; ++b) {
                    const unsigned k = zbuf[(pi * A + a) * G + pj * A + b];
                    cnt += k != EMPTY;
                    kmin = min(kmin, k);
                }
            const float m = (float)cnt * inv_a2;
            const size_t px = (size_t)(prow0 + pi) * S + pj;
            if (mask) mask[r * S * S + px] = m;
            if (depth) depth[r * S * S + px] = kmin == EMPTY ? far : depth_of(kmin);
            if (tg) {
                const float t = tg[px];
                inter += fminf(m, t);
                uni += fmaxf(m, t);
            }
        }
    }
    if (iou_sums) {
        inter = wave_sum(inter); uni = wave_sum(uni);
        if (lane == 0) { part[0][wave] = inter; part[1][wave] = uni; }
        __syncthreads();
        if (tid == 0) {
            float s0 = part[0][0], s1 = part[1][0];
            for (int w = 1; w < NT / 64; ++w) { s0 += part[0][w]; s1 += part[1][w]; }
            iou_sums[r * 2] = s0; iou_sums[r * 2 + 1] = s1;
        }
    }
}

}}  // namespace mhe::render

using namespace mhe;

extern "C" int mhe_render_mesh_f32(const float *verts, const int *faces, const float *scale, const float *trans, const float *zscale, const float *target,
                                   float *mask, float *depth, float *iou_sums, int R, int B, int V, int F, int S, int anti_aliasing, float far,
                                   void *stream) {
    MHE_REQUIRE(verts && faces && scale && trans, "mhe_render_mesh_f32: null pointer (verts, faces, scale, trans)");
    MHE_REQUIRE(mask || depth || iou_sums, "mhe_render_mesh_f32: null pointer (one of mask, depth, iou_sums is needed)");
    MHE_REQUIRE(R >= 1 && V >= 1 && F >= 1, "mhe_render_mesh_f32: R=%d V=%d F=%d (each >= 1)", R, V, F);
    MHE_REQUIRE(S >= MHE_RENDER_MIN_SIZE && S <= MHE_RENDER_MAX_SIZE, "mhe_render_mesh_f32: S=%d (S in %d..%d)", S, MHE_RENDER_MIN_SIZE, MHE_RENDER_MAX_SIZE);
    MHE_REQUIRE(!iou_sums || target, "mhe_render_mesh_f32: iou_sums needs target");
    MHE_REQUIRE(!target || (B >= 1 && R % B == 0), "mhe_render_mesh_f32: R=%d rows over B=%d target images (R must be a multiple of B >= 1)", R, B);
    MHE_REQUIRE(far == far, "mhe_render_mesh_f32: far is NaN");
    const size_t Rz = (size_t)R, img = (size_t)S * S * 4;
    struct { const void *p; size_t n; } in[6] = {{verts, Rz * V * 12}, {faces, (size_t)F * 12}, {scale, Rz * 4}, {trans, Rz * 8}, {zscale, Rz * 4},
                                                 {target, (size_t)(target ? B : 0) * img}},
                                        out[3] = {{mask, Rz * img}, {depth, Rz * img}, {iou_sums, Rz * 8}};
    for (int o = 0; o < 3; ++o) {
        for (int i = 0; i < 6; ++i)
            MHE_REQUIRE(disjoint(out[o].p, out[o].n, in[i].p, in[i].n), "mhe_render_mesh_f32: output %d overlaps input %d", o, i);
        for (int q = 0; q < o; ++q) MHE_REQUIRE(disjoint(out[o].p, out[o].n, out[q].p, out[q].n), "mhe_render_mesh_f32: outputs %d and %d overlap", q, o);
    }
    const int A = anti_aliasing ? 2 : 1, G = S * A;
    const int BR = std::min(G, render::ZW / G / A * A);            // sample rows of a band: whole pixels, what the depth words hold (G <= 512: >= 32)
    const int nbands = (G + BR - 1) / BR;
    hipLaunchKernelGGL(render::render_kernel, dim3((unsigned)R, (unsigned)(iou_sums ? 1 : nbands)), dim3(render::NT), 0, (hipStream_t)stream, verts, faces,
                       scale, trans, zscale, target, mask, depth, iou_sums, target ? B : 1, V, F, S, A, BR, nbands, far);
    return check_launch("render_kernel");
}
