// The rasteriser pieces that csrc/render.hip (mhe_render_mesh_f32) and csrc/depth_dist.hip (mhe_depth_dist_f32 and its reverse) share: the
// order-preserving depth key, the projection of a vertex to sample units, the set-up of a face and the test of one sample against it.
//   Arithmetic: a vertex is projected in f64 and rounded once to f32 sample units (<= 6e-5 of a sample spacing up to 1,024 units out);
//   edge functions and the depth plane of the rounded triangle are evaluated in f64, so no cancellation decides a sample: the
//   products are exact in f64 for coordinates of like magnitude and the sign of the difference is the true sign.  (The f32 form's error
//   grows with edge length x distance and comes within reach of a sample's 1e-3 neighbourhood for edges that cross a 512-sample image.)
#pragma once
#include "common.h"

namespace mhe { namespace raster {

__device__ __forceinline__ unsigned key_of(float d) {
    const unsigned u = __float_as_uint(d);
    return u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u);
}
__device__ __forceinline__ float depth_of(unsigned k) { return __uint_as_float(k ^ ((k >> 31) ? 0x80000000u : 0xffffffffu)); }

struct Camera {
    double s, tx, ty, half;                // |scale|, trans, G / 2
    double zs;                             // what multiplies v_z
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

// the three edge functions of sample (x, y): w0 belongs to edge a->b (the weight of c times the doubled area), w1 to b->c (a), w2 to c->a (b)
__device__ __forceinline__ void edges(const Face &f, int x, int y, double &w0, double &w1, double &w2) {
    const double px = (double)x, py = (double)y;
    w0 = fma(f.e0x, py - f.ay, -(f.e0y * (px - f.ax)));
    w1 = fma(f.e1x, py - f.by, -(f.e1y * (px - f.bx)));
    w2 = fma(f.e2x, py - f.cy, -(f.e2y * (px - f.cx)));
}

// sample (x, y) against one face: true when it is covered, d = the depth plane there, clamped to the face's range and rounded to f32
__device__ __forceinline__ bool covers(const Face &f, int x, int y, float &d) {
    const double px = (double)x, py = (double)y;
    double w0, w1, w2;
    edges(f, x, y, w0, w1, w2);
    if (!(w0 >= 0.0 && w1 >= 0.0 && w2 >= 0.0)) return false;
    d = (float)fmin(fmax(fma(f.gy, py - f.ay, fma(f.gx, px - f.ax, f.da)), f.dlo), f.dhi);
    return true;
}

}}  // namespace mhe::raster
