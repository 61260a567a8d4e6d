// Linear-blend skinning of a body model of RUNTIME size on the matrix cores (round 5): the scheme of mano_skin.hip - both products as GEMMs on
// v_mfma_f32_32x32x16_bf16 with every f32 operand split into bf16 pieces whose products are summed in f32 (blend shapes: 2 x 2 pieces, 3 products;
// per-vertex transforms: 3 x 3 pieces, 6 products; the template exact in two K slots against a coefficient of 1.0), hypothesis = MFMA row (pieces in
// LDS), vertex = column = lane (table pieces fragment-major from L2 / the Infinity Cache), 12 contiguous bytes per lane and hypothesis - for
// J <= 32 joints, any vertex count and nb shape coefficients: SMPL (24 joints, 6,890 vertices, 10 + 207 blend coefficients), the body path of
// SURVEY.md section 8 row f1 / BASELINE.json configs[4].  Reference arithmetic: hand/manopth/manolayer.py:181-188,236-246 at other sizes.
// Differences from the hand kernel: the sizes are kernel arguments (K = 9 (J - 1) + nb + 2 in KS k-steps of 16, KS even; the joints in JS = 1 or 2
// k-steps); the table pieces are made ONCE per model (mhe_lbs_split_tables_f32: they are buffers of the module, 19 MB for SMPL), not per call;
// the hypotheses' pieces take 100 KiB of LDS at SMPL's sizes, so one workgroup per CU (216 vertex tiles per workgroup: the prologue is 2 % of it).
// The scalar-operand kernel (body.hip: lbs_skin_kernel<8>, 20 TFMA/s) stays for outputs beyond 4 GiB and as MHE_LBS_MFMA=0.
#include "common.h"

namespace mhe { namespace body {

// workspace row of lbs_pose_kernel (body.hip): pose map [9(J-1)] | betas [nb] | skinning transforms [J][12] | posed joints [J][3]
__host__ __device__ inline int lws_bt(int J, int) { return 9 * (J - 1); }
__host__ __device__ inline int lws_a(int J, int nb) { return 9 * (J - 1) + nb; }
__host__ __device__ inline int lws_stride(int J, int nb) { return (9 * (J - 1) + nb + 15 * J + 15) / 16 * 16; }

typedef __attribute__((ext_vector_type(8))) __bf16 bf8;
typedef __attribute__((ext_vector_type(16))) float f32x16;
constexpr int HT = 32;

__host__ __device__ inline int lbs_ks(int J, int nb) { return ((9 * (J - 1) + nb + 2 + 15) / 16 + 1) / 2 * 2; }      // k-steps of 16, even
__host__ __device__ inline int lbs_js(int J) { return (J + 15) / 16; }
// u16 elements: PD [VT][KS][3][2][512], then W [VT][JS][3][512]
__host__ __device__ inline size_t lbs_split_pd(int VT, int KS) { return (size_t)VT * KS * 6 * 512; }
__host__ __device__ inline size_t lbs_split_elems(int VT, int KS, int JS) { return lbs_split_pd(VT, KS) + (size_t)VT * JS * 3 * 512; }

__device__ __forceinline__ void split2(float x, u16 &h, u16 &m) {
    h = f32_to_bf16(x);
    m = f32_to_bf16(x - bf16_to_f32(h));
}
__device__ __forceinline__ void split3(float x, u16 &h, u16 &m, u16 &l) {
    h = f32_to_bf16(x);
    const float r = x - bf16_to_f32(h);
    m = f32_to_bf16(r);
    l = f32_to_bf16(r - bf16_to_f32(m));
}

// the f32 vertex tables (vertex-fastest, pitch VP: body.py) -> bf16 pieces in MFMA operand order (lane l: vertex l & 31, k = 8 (l >> 5) + 0..7)
__global__ __launch_bounds__(256) void lbs_split_tables_kernel(const float *__restrict__ Vt, const float *__restrict__ Vsd, const float *__restrict__ Vpd,
                                                               const float *__restrict__ Vw, u16 *__restrict__ out, int J, int nb, int VP, int KS, int JS) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    const int lane = (int)(t & 63), v = lane & 31, kh = lane >> 5;
    const long f = t >> 6;
    const int VT = VP / 32, NP = 9 * (J - 1);
    if (f < (long)VT * KS * 3) {
        const int c = (int)(f % 3), ks = (int)((f / 3) % KS), vt = (int)(f / (3 * KS));
        u16 *o = out + ((size_t)f * 2 * 64 + lane) * 8;
        for (int j = 0; j < 8; ++j) {
            const int k = ks * 16 + kh * 8 + j;
            u16 h = 0, m = 0;
            if (k == NP + nb || k == NP + nb + 1) {          // the template against a coefficient of 1.0: (h, m), then (l, 0)
                u16 th, tm, tl;
                split3(Vt[(size_t)c * VP + vt * 32 + v], th, tm, tl);
                h = k == NP + nb ? th : tl; m = k == NP + nb ? tm : (u16)0;
            } else if (k < NP + nb) {
                const float x = k < NP ? Vpd[((size_t)k * 3 + c) * VP + vt * 32 + v] : Vsd[((size_t)(k - NP) * 3 + c) * VP + vt * 32 + v];
                split2(x, h, m);
            }
            o[j] = h; o[512 + j] = m;
        }
    } else if (f < (long)VT * KS * 3 + (long)VT * JS) {
        const long g = f - (long)VT * KS * 3;
        const int js = (int)(g % JS), vt = (int)(g / JS);
        u16 *o = out + lbs_split_pd(VT, KS) + ((size_t)g * 3 * 64 + lane) * 8;
        for (int j = 0; j < 8; ++j) {
            const int jj = js * 16 + kh * 8 + j;
            u16 h = 0, m = 0, l = 0;
            if (jj < J) split3(Vw[(size_t)jj * VP + vt * 32 + v], h, m, l);
            o[j] = h; o[512 + j] = m; o[1024 + j] = l;
        }
    }
}

#define MFMA(a, b, c) c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf8, (a)), __builtin_bit_cast(bf8, (b)), (c), 0, 0, 0)

// Keypoints (NKT > 0: NK <= 32 NKT regressor rows, kp = regressor x scaled vertices) are accumulated inside the skinning pass: a wave turns each
// finished coordinate of its 32 x 32 tile into three bf16 pieces in a private LDS tile [piece][hypothesis][vertex] (row pitch 80 bytes), reads
// them back as the A operand (hypothesis = row, vertex = k) and multiplies by the regressor's pieces for that tile (lbs_kp_split_kernel; 3 x 3
// pieces, 6 products, small terms first, as the transforms above) into 3 x NKT accumulators that stay with the wave across its vertex tiles.
// After the loop the four waves' partial sums meet in LDS and are added in the fixed order ((w0 + w1) + w2) + w3: no atomics, two launches give
// the same bits.  VERTS = false neither stores nor stages the vertices.
constexpr int KP_PITCH = 40, KP_PIECE = 32 * KP_PITCH, KP_STAGE = 3 * KP_PIECE;          // u16 elements: row, piece, one wave's tile
__host__ __device__ inline size_t lbs_kp_split_elems(int VT, int NKT) { return (size_t)VT * 2 * NKT * 3 * 512; }    // [VT][2 k-steps][NKT][3][512]

// the (NK, NV) regressor -> bf16 pieces in MFMA B-operand order (lane l: keypoint 32 nkt + (l & 31), vertex 32 vt + 16 s + 8 (l >> 5) + 0..7)
__global__ __launch_bounds__(256) void lbs_kp_split_kernel(const float *__restrict__ reg, u16 *__restrict__ out, int NK, int NV, int VT, int NKT) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    const int lane = (int)(t & 63);
    const long f = t >> 6;
    if (f >= (long)VT * 2 * NKT) return;
    const int nkt = (int)(f % NKT), s = (int)((f / NKT) & 1), vt = (int)(f / (2 * NKT));
    const int k = nkt * 32 + (lane & 31);
    u16 *o = out + ((size_t)f * 3 * 64 + lane) * 8;
    for (int j = 0; j < 8; ++j) {
        const int v = vt * 32 + s * 16 + (lane >> 5) * 8 + j;
        u16 h = 0, m = 0, l = 0;
        if (k < NK && v < NV) split3(reg[(size_t)k * NV + v], h, m, l);
        o[j] = h; o[512 + j] = m; o[1024 + j] = l;
    }
}

//
// Mesh error (ERR; NKT = 0, VERTS = false): err[r] = mean_v || scale vert[r][v] - center[r] - target[r / rpi][v] ||, accumulated inside the pass from
// the very values the vertex store would write.  The workgroup's 32 centres and target-image offsets wait in LDS (the [16][64] staging tiles of
// the vertex store are free here); a lane loads its vertex's 12 target bytes once per tile when the 32 rows share an image, per row otherwise;
// the squared difference is summed over c = 0..2, the root taken after c = 2 and added (0 for lanes without a vertex: a select, never a product
// with what was loaded) to 16 per-lane row sums that stay with the wave across its tiles.  After the loop: per wave and row the 32 vertex lanes
// in lane order, then ((w0 + w1) + w2) + w3, then one division by NV: no atomics, two launches give the same bits.
struct ErrArgs {
    const float *tgt, *center;          // [B][NV][3]; [R][3] or null (zero)
    float *err_o;                       // [R]
    int rpi;                            // rows per image (R / B)
};

template <int JS, int NKT, bool VERTS, bool ERR = false>
__device__ __forceinline__ void lbs_skin_mfma_body(const float *__restrict__ ws, const u16 *__restrict__ split, float *__restrict__ verts_o, int R, int J,
                                                   int nb, int NV, int VP, int KS, float scale, const u16 *__restrict__ ksplit,
                                                   float *__restrict__ kp_o, int NK, const ErrArgs ea = ErrArgs{nullptr, nullptr, nullptr, 1}) {
    static_assert(!ERR || (NKT == 0 && !VERTS), "the error mode neither stores vertices nor regresses keypoints");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    u16 *PMb = reinterpret_cast<u16 *>(smem);                    // [KS][2 pieces][2 k halves][32 hypotheses][8]
    u16 *Gb = PMb + (size_t)KS * 2 * 512;                        // [12 e][JS][3 pieces][2 joint halves][32][8]
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int r0 = blockIdx.x * HT;
    const int NP = 9 * (J - 1), KT = KS * 16, stride = lws_stride(J, nb), oa = lws_a(J, nb), ob = lws_bt(J, nb);
    // ---- the workgroup's hypotheses: workspace rows -> bf16 pieces in operand order (consecutive lanes: consecutive hypotheses, k rotated per
    // hypothesis so that the 32 rows' reads do not all start in one memory channel)
    for (int i = tid; i < HT * KT; i += 256) {
        const int h = i & 31;
        int kk = (i >> 5) + h;
        kk = kk >= KT ? kk - KT : kk;
        const float *w = ws + (size_t)(r0 + h < R ? r0 + h : R - 1) * stride;
        const float x = kk < NP ? w[kk] : kk < NP + nb ? w[ob + kk - NP] : kk < NP + nb + 2 ? 1.f : 0.f;
        u16 hi, mi;
        split2(x, hi, mi);
        u16 *o = PMb + ((kk >> 4) * 4 + ((kk >> 3) & 1)) * 256 + h * 8 + (kk & 7);
        o[0] = hi; o[512] = mi;
    }
    for (int i = tid; i < HT * JS * 16 * 12; i += 256) {
        const int h = i & 31, q = i >> 5, j = q / 12, e = q - j * 12;          // j < JS * 16 (joints past J: zero pieces)
        const float *w = ws + (size_t)(r0 + h < R ? r0 + h : R - 1) * stride;
        u16 hi = 0, mi = 0, lo = 0;
        if (j < J) split3(w[oa + j * 12 + e], hi, mi, lo);
        u16 *o = Gb + (((e * JS + (j >> 4)) * 3) * 2 + ((j >> 3) & 1)) * 256 + h * 8 + (j & 7);
        o[0] = hi; o[512] = mi; o[1024] = lo;
    }
    float *const Cn = reinterpret_cast<float *>(smem + (size_t)KS * 2 * 1024 + 12 * JS * 3 * 1024);          // [32][3] centres, then [32] target offsets
    unsigned *const Im = reinterpret_cast<unsigned *>(Cn + 3 * HT);
    if constexpr (ERR) {
        if (tid < 3 * HT) {
            const int h = tid / 3, r = r0 + h < R ? r0 + h : R - 1;
            Cn[tid] = ea.center ? ea.center[(size_t)r * 3 + (tid - 3 * h)] : 0.f;
        } else if (tid < 4 * HT) {
            const int h = tid - 3 * HT, r = r0 + h < R ? r0 + h : R - 1;
            Im[h] = (unsigned)(r / ea.rpi) * (unsigned)(NV * 3);
        }
    }
    __syncthreads();
    const int vl = lane & 31, half = lane >> 5;
    const bool one_image = r0 / ea.rpi == (r0 + HT - 1 < R ? r0 + HT - 1 : R - 1) / ea.rpi;          // the 32 rows share their target
    f32x16 E, SQ;
    if constexpr (ERR) {
#pragma unroll
        for (int i = 0; i < 16; ++i) E[i] = 0.f;
    }
    float *const o0 = reinterpret_cast<float *>(smem + (size_t)KS * 2 * 1024 + 12 * JS * 3 * 1024) + wave * 1024 + lane;      // [16][64] per wave
    const int hlim = R - r0 - 4 * half;                         // rows of this lane's half past the end are not stored
    const __amdgpu_buffer_rsrc_t vout = __builtin_amdgcn_make_buffer_rsrc(verts_o, 0, (int)((unsigned)R * (unsigned)(NV * 12)), 0x00020000);
    const unsigned row0 = (unsigned)r0 * (unsigned)(NV * 12);
    const int VT = VP / 32, VTL = (NV + 31) / 32;
    const uint4 *Apm = reinterpret_cast<const uint4 *>(PMb) + lane;          // + (ks * 2 + p) * 64
    const uint4 *Ag = reinterpret_cast<const uint4 *>(Gb) + lane;            // + ((e * JS + js) * 3 + p) * 64
    const uint4 *Bpd = reinterpret_cast<const uint4 *>(split) + lane;
    const uint4 *Bw = reinterpret_cast<const uint4 *>(split + lbs_split_pd(VT, KS)) + lane;
    // keypoints: this wave's staging tile (after the four waves' [16][64] stores), the regressor's pieces and the accumulators
    u16 *const St = reinterpret_cast<u16 *>(smem + (size_t)KS * 2 * 1024 + 12 * JS * 3 * 1024 + 4 * 4096) + wave * KP_STAGE;
    const uint4 *const Sa = reinterpret_cast<const uint4 *>(St) + (lane & 31) * (KP_PITCH / 8) + half;          // + p * (KP_PIECE / 8) + 2 s
    const uint4 *const Bk = reinterpret_cast<const uint4 *>(ksplit) + lane;
    f32x16 KP[3][NKT ? NKT : 1];
    if constexpr (NKT > 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int n = 0; n < NKT; ++n)
#pragma unroll
                for (int i = 0; i < 16; ++i) KP[c][n][i] = 0.f;
    }

    // table pieces: two k-steps (6 fragments each) in flight ahead of the products, running on into the wave's next tile (KS is even)
    uint4 Bf[2][6], Wp[JS][3];
    auto fetch = [&](uint4 (&f)[6], int vt, int ks) {
        const uint4 *b = Bpd + ((size_t)vt * KS + ks) * 6 * 64;
#pragma unroll
        for (int q = 0; q < 6; ++q) f[q] = b[q * 64];
    };
    if (wave < VTL) { fetch(Bf[0], wave, 0); fetch(Bf[1], wave, 1); }
    for (int vt = wave; vt < VTL; vt += 4) {
#pragma unroll
        for (int js = 0; js < JS; ++js)
#pragma unroll
            for (int p = 0; p < 3; ++p) Wp[js][p] = Bw[((vt * JS + js) * 3 + p) * 64];
        uint4 Kf[2][NKT ? NKT : 1][3];
        if constexpr (NKT > 0) {
#pragma unroll
            for (int s = 0; s < 2; ++s)
#pragma unroll
                for (int n = 0; n < NKT; ++n)
#pragma unroll
                    for (int p = 0; p < 3; ++p) Kf[s][n][p] = Bk[(((size_t)(vt * 2 + s) * NKT + n) * 3 + p) * 64];
        }
        const unsigned tv = (unsigned)((vt * 32 + vl < NV ? vt * 32 + vl : NV - 1) * 3);          // lanes without a vertex re-read the last one
        float tg[3] = {0.f, 0.f, 0.f};
        if constexpr (ERR) {
            if (one_image) {
#pragma unroll
                for (int c = 0; c < 3; ++c) tg[c] = ea.tgt[Im[0] + tv + c];
            }
        }
        f32x16 X[3];
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int i = 0; i < 16; ++i) X[c][i] = 0.f;
        const int vn = vt + 4 < VTL ? vt + 4 : vt;                // (the last tile re-fetches its own first k-steps: nothing reads them)
        for (int ks = 0; ks < KS; ks += 2) {
#pragma unroll
            for (int d = 0; d < 2; ++d) {
                const uint4 ah = Apm[((ks + d) * 2 + 0) * 64], am = Apm[((ks + d) * 2 + 1) * 64];
#pragma unroll
                for (int c = 0; c < 3; ++c) { MFMA(am, Bf[d][2 * c], X[c]); MFMA(ah, Bf[d][2 * c + 1], X[c]); MFMA(ah, Bf[d][2 * c], X[c]); }
                __builtin_amdgcn_sched_barrier(0);
                if (ks + d + 2 < KS) fetch(Bf[d], vt, ks + d + 2);
                else fetch(Bf[d], vn, ks + d + 2 - KS);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        const int v = vt * 32 + vl;
        // the lane's part of the address (the rest is wave-uniform: SGPR offset); lanes without a vertex and rows past R get an offset the
        // buffer's range check rejects (it looks at the VGPR offset)
        const unsigned voff = v < NV ? (unsigned)((4 * half * NV + v) * 12) : 0xffffffffu;
#pragma unroll
        for (int c = 0; c < 3; ++c) {            // one output coordinate at a time: four transform entries live instead of twelve
            f32x16 T[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int e = q < 3 ? 3 * c + q : 9 + c;
#pragma unroll
                for (int i = 0; i < 16; ++i) T[q][i] = 0.f;
#pragma unroll
                for (int js = 0; js < JS; ++js) {
                    const uint4 gh = Ag[((e * JS + js) * 3 + 0) * 64], gm = Ag[((e * JS + js) * 3 + 1) * 64], gl = Ag[((e * JS + js) * 3 + 2) * 64];
                    MFMA(gh, Wp[js][2], T[q]); MFMA(gl, Wp[js][0], T[q]); MFMA(gm, Wp[js][1], T[q]);           // small terms first
                    MFMA(gh, Wp[js][1], T[q]); MFMA(gm, Wp[js][0], T[q]); MFMA(gh, Wp[js][0], T[q]);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
            // v' = T [X; 1] (manolayer.py:236-246), x scale; 8 + 4 bytes of the lane's 12 per hypothesis (the first coordinate waits in LDS)
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int hr = (i & 3) + 8 * (i >> 2);                    // (+ 4 * half) the accumulator's row = hypothesis within the workgroup
                const float r = affine_row(T[0][i], X[0][i], T[1][i], X[1][i], T[2][i], X[2][i], T[3][i], scale);
                const unsigned soff = row0 + (unsigned)(hr * NV * 12);
                if constexpr (NKT > 0) {
                    u16 ph, pm, pl;
                    split3(r, ph, pm, pl);
                    u16 *o = St + (hr + 4 * half) * KP_PITCH + vl;
                    o[0] = ph; o[KP_PIECE] = pm; o[2 * KP_PIECE] = pl;
                }
                if constexpr (VERTS) {
                    if (c == 0) o0[i * 64] = r;
                    else if (c == 1) {
                        typedef __attribute__((ext_vector_type(2))) unsigned u32x2;
                        const u32x2 o = {__float_as_uint(o0[i * 64]), __float_as_uint(r)};
                        __builtin_amdgcn_raw_buffer_store_b64(o, vout, (int)(hr < hlim ? voff : 0xffffffffu), (int)soff, 0);
                    } else __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(r), vout, (int)(hr < hlim ? voff : 0xffffffffu), (int)(soff + 8u), 0);
                }
            }
            if constexpr (ERR) {
                // the same affine_row on the same operands as the store above; a real branch, so that the 16 per-row loads are issued only where
                // the rows do not share an image and one coordinate at a time
                auto add = [&](int i, float t) {
                    const int hr = (i & 3) + 8 * (i >> 2) + 4 * half;
                    const float r = affine_row(T[0][i], X[0][i], T[1][i], X[1][i], T[2][i], X[2][i], T[3][i], scale);
                    const float d = (r - Cn[hr * 3 + c]) - t;
                    SQ[i] = c == 0 ? d * d : __builtin_fmaf(d, d, SQ[i]);
                    if (c == 2) E[i] += v < NV ? __builtin_sqrtf(SQ[i]) : 0.f;
                };
                if (one_image) {
#pragma unroll
                    for (int i = 0; i < 16; ++i) add(i, tg[c]);
                } else {
#pragma unroll
                    for (int i = 0; i < 16; ++i) add(i, ea.tgt[Im[(i & 3) + 8 * (i >> 2) + 4 * half] + tv + c]);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
            if constexpr (NKT > 0) {
                wave_sync();                     // the tile is the wave's own: its DS operations complete in order
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    const uint4 ah = Sa[2 * s], am = Sa[KP_PIECE / 8 + 2 * s], al = Sa[2 * (KP_PIECE / 8) + 2 * s];
#pragma unroll
                    for (int n = 0; n < NKT; ++n) {
                        MFMA(ah, Kf[s][n][2], KP[c][n]); MFMA(al, Kf[s][n][0], KP[c][n]); MFMA(am, Kf[s][n][1], KP[c][n]);       // small terms first
                        MFMA(ah, Kf[s][n][1], KP[c][n]); MFMA(am, Kf[s][n][0], KP[c][n]); MFMA(ah, Kf[s][n][0], KP[c][n]);
                    }
                }
                wave_sync();                     // (the next coordinate overwrites the tile)
            }
        }
    }
    if constexpr (NKT > 0) {
        // the four waves' partial sums: [wave][c][keypoint][hypothesis, pitch 33] over the hypotheses' pieces (every wave is past its last tile)
        __syncthreads();
        float *P = reinterpret_cast<float *>(smem);
        constexpr int PW = 3 * NKT * 32 * 33;
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int n = 0; n < NKT; ++n)
#pragma unroll
                for (int i = 0; i < 16; ++i)
                    P[wave * PW + ((c * NKT + n) * 32 + vl) * 33 + (i & 3) + 8 * (i >> 2) + 4 * half] = KP[c][n][i];
        __syncthreads();
        for (int i = tid; i < HT * NK * 3; i += 256) {
            const int h = i / (NK * 3), e = i - h * NK * 3, k = e / 3, c = e - 3 * k;
            const float *q = P + (c * NKT * 32 + k) * 33 + h;
            if (r0 + h < R) kp_o[(size_t)(r0 + h) * NK * 3 + e] = ((q[0] + q[PW]) + q[2 * PW]) + q[3 * PW];
        }
    }
    if constexpr (ERR) {
        // [wave][row][vertex lane, pitch 33] over the hypotheses' pieces (every wave is past its last tile), then [wave][row] behind it
        __syncthreads();
        float *P = reinterpret_cast<float *>(smem), *S = P + 4 * HT * 33;
#pragma unroll
        for (int i = 0; i < 16; ++i) P[(wave * HT + (i & 3) + 8 * (i >> 2) + 4 * half) * 33 + vl] = E[i];
        __syncthreads();
        if (tid < 4 * HT) {
            const float *q = P + tid * 33;
            float a = q[0];
            for (int l = 1; l < 32; ++l) a += q[l];
            S[tid] = a;
        }
        __syncthreads();
        if (tid < HT && r0 + tid < R) ea.err_o[r0 + tid] = (((S[tid] + S[HT + tid]) + S[2 * HT + tid]) + S[3 * HT + tid]) / (float)NV;
    }
}

template <int JS>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2)))
void lbs_skin_mfma_kernel(const float *__restrict__ ws, const u16 *__restrict__ split, float *__restrict__ verts_o, int R, int J, int nb, int NV, int VP,
                          int KS, float scale) {
    lbs_skin_mfma_body<JS, 0, true>(ws, split, verts_o, R, J, nb, NV, VP, KS, scale, nullptr, nullptr, 0);
}

// the mesh-error variant: one workgroup per CU (LDS), one wave per SIMD as the keypoint variants (at two waves the 32 extra accumulator
// registers and the per-row target loads spill)
template <int JS>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1)))
void lbs_skin_err_mfma_kernel(const float *__restrict__ ws, const u16 *__restrict__ split, const float *__restrict__ tgt, const float *__restrict__ center,
                              float *__restrict__ err_o, int R, int J, int nb, int NV, int VP, int KS, int rpi, float scale) {
    lbs_skin_mfma_body<JS, 0, false, true>(ws, split, nullptr, R, J, nb, NV, VP, KS, scale, nullptr, nullptr, 0, ErrArgs{tgt, center, err_o, rpi});
}

// the keypoint variants: one workgroup per CU either way (LDS), so one wave per SIMD and the whole register file (the accumulators in AGPRs)
template <int JS, int NKT, bool VERTS>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1)))
void lbs_skin_kp_mfma_kernel(const float *__restrict__ ws, const u16 *__restrict__ split, const u16 *__restrict__ ksplit, float *__restrict__ verts_o,
                             float *__restrict__ kp_o, int R, int J, int nb, int NV, int VP, int KS, int NK, float scale) {
    lbs_skin_mfma_body<JS, NKT, VERTS>(ws, split, verts_o, R, J, nb, NV, VP, KS, scale, ksplit, kp_o, NK);
}

}}  // namespace mhe::body

using namespace mhe;

extern "C" size_t mhe_lbs_split_floats(int J, int nb, int VP) {
    if (J <= 0 || J > 32 || nb < 0 || VP <= 0 || VP % 32) return 0;
    return (body::lbs_split_elems(VP / 32, body::lbs_ks(J, nb), body::lbs_js(J)) * sizeof(u16) + 3) / 4;
}

extern "C" int mhe_lbs_split_tables_f32(const float *v_template, const float *v_shapedirs, const float *v_posedirs, const float *v_weights,
                                        float *split, int J, int nb, int VP, void *stream) {
    MHE_REQUIRE(v_template && v_shapedirs && v_posedirs && v_weights && split, "mhe_lbs_split_tables_f32: null pointer");
    MHE_REQUIRE(J > 0 && J <= 32 && nb > 0 && VP > 0 && VP % 32 == 0, "mhe_lbs_split_tables_f32: J=%d nb=%d VP=%d (VP a multiple of 32)", J, nb, VP);
    const int KS = body::lbs_ks(J, nb), JS = body::lbs_js(J), VT = VP / 32;
    const long frags = (long)VT * KS * 3 + (long)VT * JS;
    hipLaunchKernelGGL(body::lbs_split_tables_kernel, dim3((unsigned)((frags * 64 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, v_template,
                       v_shapedirs, v_posedirs, v_weights, reinterpret_cast<u16 *>(split), J, nb, VP, KS, JS);
    return check_launch("lbs_split_tables_kernel");
}

extern "C" int mhe_lbs_skin_mfma_supported(int R, int J, int nb, int NV, int VP) {
    if (R <= 0 || J <= 0 || J > 32 || nb <= 0 || NV <= 0 || VP < NV || VP % 32) return 0;
    if ((size_t)(R + 64) * NV * 12 >= (1ull << 32)) return 0;                                   // 32-bit byte offsets of the output
    const size_t lds = (size_t)body::lbs_ks(J, nb) * 2048 + (size_t)12 * body::lbs_js(J) * 3072 + 4 * 4096;
    return lds <= 160 * 1024;
}

extern "C" int mhe_lbs_skin_mfma_f32(const float *workspace, const float *split, float *verts, int R, int J, int nb, int NV, int VP, float scale,
                                     void *stream) {
    MHE_REQUIRE(workspace && split && verts, "mhe_lbs_skin_mfma_f32: null pointer");
    MHE_REQUIRE(mhe_lbs_skin_mfma_supported(R, J, nb, NV, VP), "mhe_lbs_skin_mfma_f32: R=%d J=%d nb=%d NV=%d VP=%d not supported (see mhe_lbs_skin_mfma_supported)",
                R, J, nb, NV, VP);
    const int KS = body::lbs_ks(J, nb), JS = body::lbs_js(J);
    const int lds = KS * 2048 + 12 * JS * 3072 + 4 * 4096;
    const dim3 grid((unsigned)((R + body::HT - 1) / body::HT));
    if (JS == 1) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(body::lbs_skin_mfma_kernel<1>), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
        hipLaunchKernelGGL(body::lbs_skin_mfma_kernel<1>, grid, dim3(256), lds, (hipStream_t)stream, workspace, reinterpret_cast<const u16 *>(split), verts,
                           R, J, nb, NV, VP, KS, scale);
    } else {
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(body::lbs_skin_mfma_kernel<2>), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
        hipLaunchKernelGGL(body::lbs_skin_mfma_kernel<2>, grid, dim3(256), lds, (hipStream_t)stream, workspace, reinterpret_cast<const u16 *>(split), verts,
                           R, J, nb, NV, VP, KS, scale);
    }
    return check_launch("lbs_skin_mfma_kernel");
}

extern "C" size_t mhe_lbs_kp_split_floats(int NK, int VP) {
    if (NK < 1 || NK > 64 || VP <= 0 || VP % 32) return 0;
    return (body::lbs_kp_split_elems(VP / 32, (NK + 31) / 32) * sizeof(u16) + 3) / 4;
}

extern "C" int mhe_lbs_kp_split_tables_f32(const float *regressor, float *ksplit, int NK, int NV, int VP, void *stream) {
    MHE_REQUIRE(regressor && ksplit, "mhe_lbs_kp_split_tables_f32: null pointer");
    MHE_REQUIRE(NK >= 1 && NK <= 64 && NV > 0 && VP >= NV && VP % 32 == 0, "mhe_lbs_kp_split_tables_f32: NK=%d (1..64) NV=%d VP=%d (VP >= NV, a multiple of 32)",
                NK, NV, VP);
    const int VT = VP / 32, NKT = (NK + 31) / 32;
    const long frags = (long)VT * 2 * NKT;
    hipLaunchKernelGGL(body::lbs_kp_split_kernel, dim3((unsigned)((frags * 64 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, regressor,
                       reinterpret_cast<u16 *>(ksplit), NK, NV, VT, NKT);
    return check_launch("lbs_kp_split_kernel");
}

static size_t lbs_kp_lds(int J, int nb, int NK) {
    const size_t skin = (size_t)body::lbs_ks(J, nb) * 2048 + (size_t)12 * body::lbs_js(J) * 3072 + 4 * 4096 + 4 * body::KP_STAGE * sizeof(u16);
    const size_t sums = (size_t)4 * 3 * ((NK + 31) / 32) * 32 * 33 * sizeof(float);
    return skin > sums ? skin : sums;
}

extern "C" int mhe_lbs_skin_kp_supported(int R, int J, int nb, int NV, int VP, int NK, int want_verts) {
    if (R <= 0 || J <= 0 || J > 32 || nb <= 0 || NV <= 0 || VP < NV || VP % 32 || NK < 1 || NK > 64) return 0;
    if (want_verts && (size_t)(R + 64) * NV * 12 >= (1ull << 32)) return 0;                     // 32-bit byte offsets of the vertex output
    return lbs_kp_lds(J, nb, NK) <= 160 * 1024;
}

template <int JS, int NKT, bool VERTS>
static void launch_skin_kp(const float *ws, const u16 *split, const u16 *ksplit, float *verts, float *kp, int R, int J, int nb, int NV, int VP, int NK,
                           float scale, hipStream_t stream) {
    const int lds = (int)lbs_kp_lds(J, nb, NK);
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(body::lbs_skin_kp_mfma_kernel<JS, NKT, VERTS>), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    hipLaunchKernelGGL((body::lbs_skin_kp_mfma_kernel<JS, NKT, VERTS>), dim3((unsigned)((R + body::HT - 1) / body::HT)), dim3(256), lds, stream, ws, split,
                       ksplit, verts, kp, R, J, nb, NV, VP, body::lbs_ks(J, nb), NK, scale);
}

extern "C" int mhe_lbs_skin_kp_mfma_f32(const float *workspace, const float *split, const float *ksplit, float *verts, float *keypoints, int R, int J,
                                        int nb, int NV, int VP, int NK, float scale, void *stream) {
    MHE_REQUIRE(NK >= 1 && NK <= 64, "mhe_lbs_skin_kp_mfma_f32: NK=%d outside 1..64", NK);
    MHE_REQUIRE(workspace && split && ksplit && keypoints, "mhe_lbs_skin_kp_mfma_f32: null pointer (only verts may be null)");
    MHE_REQUIRE(mhe_lbs_skin_kp_supported(R, J, nb, NV, VP, NK, verts != nullptr),
                "mhe_lbs_skin_kp_mfma_f32: R=%d J=%d nb=%d NV=%d VP=%d NK=%d not supported (see mhe_lbs_skin_kp_supported)", R, J, nb, NV, VP, NK);
    const u16 *sp = reinterpret_cast<const u16 *>(split), *ks = reinterpret_cast<const u16 *>(ksplit);
    hipStream_t st = (hipStream_t)stream;
    const int JS = body::lbs_js(J), NKT = (NK + 31) / 32;
#define MHE_KP_LAUNCH(js, nkt)                                                                                      \
    do {                                                                                                            \
        if (verts) launch_skin_kp<js, nkt, true>(workspace, sp, ks, verts, keypoints, R, J, nb, NV, VP, NK, scale, st); \
        else launch_skin_kp<js, nkt, false>(workspace, sp, ks, verts, keypoints, R, J, nb, NV, VP, NK, scale, st);      \
    } while (0)
    if (JS == 1 && NKT == 1) MHE_KP_LAUNCH(1, 1);
    else if (JS == 1) MHE_KP_LAUNCH(1, 2);
    else if (NKT == 1) MHE_KP_LAUNCH(2, 1);
    else MHE_KP_LAUNCH(2, 2);
#undef MHE_KP_LAUNCH
    return check_launch("lbs_skin_kp_mfma_kernel");
}

extern "C" int mhe_lbs_skin_err_supported(int R, int J, int nb, int NV, int VP, int B) {
    if (R <= 0 || J <= 0 || J > 32 || nb <= 0 || NV <= 0 || VP < NV || VP % 32 || B <= 0 || R % B) return 0;
    if ((size_t)B * NV * 3 >= (1ull << 31)) return 0;                                           // 32-bit element offsets into the targets
    const size_t lds = (size_t)body::lbs_ks(J, nb) * 2048 + (size_t)12 * body::lbs_js(J) * 3072 + 4 * 4096;
    return lds <= 160 * 1024;
}

extern "C" int mhe_lbs_skin_err_mfma_f32(const float *workspace, const float *split, const float *target_verts, const float *center, float *err, int R,
                                         int B, int J, int nb, int NV, int VP, float scale, void *stream) {
    MHE_REQUIRE(workspace && split && target_verts && err, "mhe_lbs_skin_err_mfma_f32: null pointer (only center may be null)");
    MHE_REQUIRE(mhe_lbs_skin_err_supported(R, J, nb, NV, VP, B),
                "mhe_lbs_skin_err_mfma_f32: R=%d B=%d J=%d nb=%d NV=%d VP=%d not supported (see mhe_lbs_skin_err_supported)", R, B, J, nb, NV, VP);
    const int KS = body::lbs_ks(J, nb), JS = body::lbs_js(J);
    const int lds = KS * 2048 + 12 * JS * 3072 + 4 * 4096;          // the plain kernel's: the sums (4 x 32 x 34 floats) fit over the pieces
    const dim3 grid((unsigned)((R + body::HT - 1) / body::HT));
    const u16 *sp = reinterpret_cast<const u16 *>(split);
    if (JS == 1) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(body::lbs_skin_err_mfma_kernel<1>), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
        hipLaunchKernelGGL(body::lbs_skin_err_mfma_kernel<1>, grid, dim3(256), lds, (hipStream_t)stream, workspace, sp, target_verts, center, err, R, J, nb,
                           NV, VP, KS, R / B, scale);
    } else {
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(body::lbs_skin_err_mfma_kernel<2>), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
        hipLaunchKernelGGL(body::lbs_skin_err_mfma_kernel<2>, grid, dim3(256), lds, (hipStream_t)stream, workspace, sp, target_verts, center, err, R, J, nb,
                           NV, VP, KS, R / B, scale);
    }
    return check_launch("lbs_skin_err_mfma_kernel");
}
