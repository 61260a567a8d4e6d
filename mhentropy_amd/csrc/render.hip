// Silhouette and depth of a triangle mesh under the orthographic camera of the 2D head (ManoLayer.render, ops.render_mesh,
// criteria.silhouette_iou): mhe_render_mesh_f32.  The contract is the one written at the entry's declaration in include/mhe.h.
//   One workgroup renders one row band of one hypothesis into a depth image in LDS: a word per sample holds the order-preserving integer
//   image of the nearest depth (EMPTY where nothing covers), faces are thrown at it with atomicMin - coverage and depth do not depend on the
//   order in which faces arrive.  A thread takes a face: bounding box clamped to the band, every sample of the box tested.  A face whose box
//   holds BIG samples or more is put on a list and rasterised by the whole workgroup afterwards (a face that covers the image would
//   otherwise keep one thread busy for 16k samples).  The pixels are then resolved from LDS: mask = covered samples / A^2, depth = nearest
//   covered sample, and min / max against the target summed in a fixed order - the mask need not be written at all.
//   Arithmetic: a vertex is projected in f64 and rounded once to f32 sample units (<= 6e-5 of a sample spacing up to 1,024 units out);
//   edge functions and the depth plane of the rounded triangle are evaluated in f64, so no cancellation decides a sample: the
//   products are exact in f64 for coordinates of like magnitude and the sign of the difference is the true sign.  (The f32 form's error
//   grows with edge length x distance and comes within reach of a sample's 1e-3 neighbourhood for edges that cross a 512-sample image.)
#include <algorithm>
#include "common.h"

namespace mhe { namespace render {

constexpr int NT = 512;                    // threads of a workgroup
constexpr int ZW = 16384;                  // depth words of one band (64 KiB): a 64 x 64 anti-aliased image whole
constexpr int VS = 1024;                   // vertices staged in LDS (12 KiB); a larger mesh projects its vertices per face from global memory
constexpr int BIG = 64, NBIG = 256;        // samples in the clamped box from which a face goes to the workgroup's list; its length
constexpr unsigned EMPTY = 0xffffffffu;    // above the image of every number (+inf is 0xff800000)
// two workgroups per CU: 2 (64 + 12 + 1 KiB and a few words) < 160 KiB

__device__ __forceinline__ unsigned key_of(float d) {
    const unsigned u = __float_as_uint(d);
    return u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u);
}
__device__ __forceinline__ float depth_of(unsigned k) { return __uint_as_float(k ^ ((k >> 31) ? 0x80000000u : 0xffffffffu)); }

struct Camera {
    double s, tx, ty, half;                // |scale|, trans, G / 2
    double zs;                             // zscale / 1000, or 1
};

// sample (row i, col j) sits at x = (2 j + 1) / G - 1: column coordinate X = (x + 1) G / 2 - 1 / 2 puts sample j at X = j
__device__ __forceinline__ void project(const float *v, const Camera &c, float &X, float &Y, float &D) {
    X = (float)(fma(fma(c.s, (double)v[0], c.tx), c.half, c.half) - 0.5);
    Y = (float)(fma(fma(c.s, (double)v[1], c.ty), c.half, c.half) - 0.5);
    D = (float)((double)v[2] * c.zs);
}

struct Face {
    double ax, ay, bx, by, cx, cy;         // the rounded projected vertices, sample units
    double e0x, e0y, e1x, e1y, e2x, e2y;   // edges a->b, b->c, c->a, oriented so that the inside is >= 0 on all three
    double da, gx, gy, dlo, dhi;           // depth plane through a; the face's depth range
    int x0, x1, y0, y1;                    // the box, clamped to the band
};

struct Band {
    int G, y0, y1;                         // samples per row; first and last sample row of the band
};

// false: the face covers nothing in this band (an index outside [0, V), which is never followed; zero or non-finite projected area; box off the band)
__device__ __forceinline__ bool setup(Face &f, int face, const int *__restrict__ faces, const float *__restrict__ vr, int V, bool staged, const float *sx,
                                      const float *sy, const float *sd, const Camera &cam, const Band &bd) {
    const int i0 = faces[(size_t)face * 3], i1 = faces[(size_t)face * 3 + 1], i2 = faces[(size_t)face * 3 + 2];
    if ((unsigned)i0 >= (unsigned)V || (unsigned)i1 >= (unsigned)V || (unsigned)i2 >= (unsigned)V) return false;
    float ax, ay, ad, bx, by, bdp, cx, cy, cd;
    if (staged) {
        ax = sx[i0]; ay = sy[i0]; ad = sd[i0]; bx = sx[i1]; by = sy[i1]; bdp = sd[i1]; cx = sx[i2]; cy = sy[i2]; cd = sd[i2];
    } else {
        project(vr + (size_t)i0 * 3, cam, ax, ay, ad); project(vr + (size_t)i1 * 3, cam, bx, by, bdp); project(vr + (size_t)i2 * 3, cam, cx, cy, cd);
    }
    // the box in float, clamped before it becomes integers (a NaN fails the comparison and drops the face)
    const float x0 = fmaxf(ceilf(fminf(ax, fminf(bx, cx))), 0.f), x1 = fminf(floorf(fmaxf(ax, fmaxf(bx, cx))), (float)(bd.G - 1));
    const float y0 = fmaxf(ceilf(fminf(ay, fminf(by, cy))), (float)bd.y0), y1 = fminf(floorf(fmaxf(ay, fmaxf(by, cy))), (float)bd.y1);
    if (!(x0 <= x1 && y0 <= y1)) return false;
    const double abx = (double)bx - ax, aby = (double)by - ay, acx = (double)cx - ax, acy = (double)cy - ay;
    const double area = fma(abx, acy, -(aby * acx));
    if (!(fabs(area) > 0.0 && fabs(area) < __builtin_inf())) return false;
    const double sg = area > 0.0 ? 1.0 : -1.0, inv = 1.0 / area, dab = (double)bdp - ad, dac = (double)cd - ad;
    f.ax = ax; f.ay = ay; f.bx = bx; f.by = by; f.cx = cx; f.cy = cy;
    f.e0x = sg * abx; f.e0y = sg * aby;
    f.e1x = sg * ((double)cx - bx); f.e1y = sg * ((double)cy - by);
    f.e2x = sg * -acx; f.e2y = sg * -acy;
    f.da = ad;
    f.gx = fma(dab, acy, -(dac * aby)) * inv;
    f.gy = fma(dac, abx, -(dab * acx)) * inv;
    f.dlo = fminf(ad, fminf(bdp, cd)); f.dhi = fmaxf(ad, fmaxf(bdp, cd));
    f.x0 = (int)x0; f.x1 = (int)x1; f.y0 = (int)y0; f.y1 = (int)y1;
    return true;
}

// sample (x, y) of the band against one face; x in [0, G), y in [band.y0, band.y1]
__device__ __forceinline__ void shade(const Face &f, int x, int y, const Band &bd, unsigned *zbuf) {
    const double px = (double)x, py = (double)y;
    const double w0 = fma(f.e0x, py - f.ay, -(f.e0y * (px - f.ax)));
    const double w1 = fma(f.e1x, py - f.by, -(f.e1y * (px - f.bx)));
    const double w2 = fma(f.e2x, py - f.cy, -(f.e2y * (px - f.cx)));
    if (w0 >= 0.0 && w1 >= 0.0 && w2 >= 0.0) {
        const double d = fmin(fmax(fma(f.gy, py - f.ay, fma(f.gx, px - f.ax, f.da)), f.dlo), f.dhi);
        atomicMin(&zbuf[(y - bd.y0) * bd.G + x], key_of((float)d));
    }
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
