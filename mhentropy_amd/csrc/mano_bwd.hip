// Reverse mode of the MANO loss pass: d(sum_r g_r * log_p_r) / d(th45, det) for every hypothesis row,
// one wavefront per hypothesis.  The wave first re-runs joint_pass (forward values stay in its LDS scratch),
// then walks the chain backwards keeping all adjoints in a second per-wave LDS scratch:
//   Laplace likelihood + soft priors  (hand/network.py:155-165,233-258,612-667)
//   orthographic projection            (hand/network.py:497-514)
//   root/bone normalisation            (hand/utils.py:46-66)
//   reorder / centre / mm              (hand/manopth/manolayer.py:260-273, hand/ManoLayer.py:54-56)
//   fingertip skinning + blend shapes  (manolayer.py:181-188,236-251)
//   kinematic chain                    (manolayer.py:193-234)
//   Rodrigues through the quaternion   (rodrigues_layer.py:15-54)
//   PCA pose coefficients              (manolayer.py:131-143)
// It stands where autograd differentiates those lines in the reference's train step
// (hand/CrossModalHand.py:455-470 `loss.backward()`).
#include "mano_joint_pass.h"

namespace mhe { namespace mano {

// adjoint scratch per wave (floats)
constexpr int A_ROT = 0;       // [16][9]   local rotations
constexpr int A_JR = 144;      // [16][3]   rest joints
constexpr int A_G = 192;       // [16][12]  global rotation (9) + joint position (3)
constexpr int A_GR = 384;      // [16][12]  skinning transform
constexpr int A_PRE = 576;     // [21][3]   chain joints + skinned tips (metres, pre-reorder)
constexpr int A_TIPV = 640;    // [5][3]    posed tip vertices (rest frame)
constexpr int A_POSE = 656;    // [48]      axis-angles
constexpr int A_SCRATCH = 704;

// Reverse of joint_pass from the pre-reorder joints back to the pose: ad[A_PRE] (adjoints of the 16 chain joints and the 5 skinned tips, metres)
// -> ad[A_POSE] (the 48 axis-angles); returns the beta adjoint on lanes < 10.  sc holds joint_pass' forward values of the row.
// SEED (the full-mesh reverse, mano_verts_bwd_kernel): `seed` is the row's adjoint record of the skinning reverse in the workspace row's layout
// (mano_layout.h) - its transforms join A_GR, its pose map the local rotations (pose map = R_j - I, j >= 1), its betas the beta adjoint.
// Ends on a wave_sync: the caller may read ad[A_POSE].
template <bool SEED>
__device__ __forceinline__ float joint_chain_bwd(const float *tb, const float *sc, float *ad, int lane, const float *__restrict__ seed) {
    // ---- fingertip skinning  v' = sum_j w_j (Gr_j [v;1])
    if (lane < 15) {
        const int tip = lane / 3, d = lane % 3;
        float ap = 0.f;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float T = 0.f;
#pragma unroll
            for (int j = 0; j < 16; ++j) T = fmaf(tb[TIP_W + tip * 16 + j], sc[S_GR + 12 * j + 3 * c + d], T);
            ap = fmaf(ad[A_PRE + 48 + 3 * tip + c], T, ap);
        }
        ad[A_TIPV + lane] = ap;
    }
    for (int e = lane; e < 192; e += 64) {
        const int j = e / 12, q = e % 12;
        float acc = 0.f;
#pragma unroll
        for (int tip = 0; tip < 5; ++tip) {
            const float av = ad[A_PRE + 48 + 3 * tip + (q < 9 ? q / 3 : q - 9)];
            acc = fmaf(tb[TIP_W + tip * 16 + j] * av, q < 9 ? sc[S_TIPV + 3 * tip + q % 3] : 1.f, acc);
        }
        if constexpr (SEED) acc += seed[WS_GR + e];
        ad[A_GR + e] = acc;
        ad[A_G + e] = q < 9 ? 0.f : ad[A_PRE + 3 * j + (q - 9)];      // chain joints are the transforms' translations
    }
    wave_sync();
    // ---- blend shapes of the tips: pose-corrective -> local rotations, shape -> beta
    for (int k = lane; k < 144; k += 64) {
        float a = 0.f;
        if (k >= 9) {
#pragma unroll
            for (int tc = 0; tc < 15; ++tc) a = fmaf(tb[TIP_PD + tc * 135 + (k - 9)], ad[A_TIPV + tc], a);
            if constexpr (SEED) a += seed[WS_PM + k - 9];
        }
        ad[A_ROT + k] = a;
    }
    float a_beta = 0.f;
    if (lane < 10) {
#pragma unroll
        for (int tc = 0; tc < 15; ++tc) a_beta = fmaf(tb[TIP_SD + tc * 10 + lane], ad[A_TIPV + tc], a_beta);
        if constexpr (SEED) a_beta += seed[WS_BT + lane];
    }
    // ---- Gr_j = [Rg_j | t_j - Rg_j jr_j]
    if (lane < 16) {
        const int j = lane;
        const float *Rg = sc + S_G + 12 * j, *jr = sc + S_JR + 3 * j;
        float atr[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) atr[c] = ad[A_GR + 12 * j + 9 + c];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            ad[A_G + 12 * j + 9 + c] += atr[c];
#pragma unroll
            for (int d = 0; d < 3; ++d) ad[A_G + 12 * j + 3 * c + d] += ad[A_GR + 12 * j + 3 * c + d] - atr[c] * jr[d];
            ad[A_JR + 3 * j + c] = -(Rg[c] * atr[0] + Rg[3 + c] * atr[1] + Rg[6 + c] * atr[2]);
        }
    }
    wave_sync();
    // ---- kinematic chain, tips of the fingers back to the wrist; one finger per lane
    float rootv[15];
#pragma unroll
    for (int e = 0; e < 15; ++e) rootv[e] = 0.f;
    if (lane < 5) {
#pragma unroll
        for (int lvl = 2; lvl >= 0; --lvl) {
            const int j = 1 + 3 * lane + lvl, parent = lvl ? j - 1 : 0;
            float PR[9], Rj[9], aRg[9], at[3], rel[3], aPR[9], arel[3];
#pragma unroll
            for (int e = 0; e < 9; ++e) { PR[e] = sc[S_G + 12 * parent + e]; Rj[e] = sc[S_ROT + 9 * j + e]; aRg[e] = ad[A_G + 12 * j + e]; }
#pragma unroll
            for (int c = 0; c < 3; ++c) { at[c] = ad[A_G + 12 * j + 9 + c]; rel[c] = sc[S_JR + 3 * j + c] - sc[S_JR + 3 * parent + c]; }
#pragma unroll
            for (int a = 0; a < 3; ++a)
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    // Rg_j = PR Rj ;  t_j = PR rel + t_parent
                    ad[A_ROT + 9 * j + 3 * a + k] += PR[a] * aRg[k] + PR[3 + a] * aRg[3 + k] + PR[6 + a] * aRg[6 + k];
                    aPR[3 * a + k] = aRg[3 * a] * Rj[3 * k] + aRg[3 * a + 1] * Rj[3 * k + 1] + aRg[3 * a + 2] * Rj[3 * k + 2] + at[a] * rel[k];
                }
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                arel[k] = PR[k] * at[0] + PR[3 + k] * at[1] + PR[6 + k] * at[2];
                ad[A_JR + 3 * j + k] += arel[k];
            }
            if (lvl) {
#pragma unroll
                for (int e = 0; e < 9; ++e) ad[A_G + 12 * parent + e] += aPR[e];
#pragma unroll
                for (int c = 0; c < 3; ++c) { ad[A_G + 12 * parent + 9 + c] += at[c]; ad[A_JR + 3 * parent + c] -= arel[c]; }
            } else {
#pragma unroll
                for (int e = 0; e < 9; ++e) rootv[e] = aPR[e];
#pragma unroll
                for (int c = 0; c < 3; ++c) { rootv[9 + c] = at[c]; rootv[12 + c] = -arel[c]; }
            }
        }
    }
#pragma unroll
    for (int e = 0; e < 15; ++e) rootv[e] = wave_sum(rootv[e]);
    if (lane == 0) {
        // wrist: Rg_0 = R_0, t_0 = jr_0
#pragma unroll
        for (int e = 0; e < 9; ++e) ad[A_ROT + e] += ad[A_G + e] + rootv[e];
#pragma unroll
        for (int c = 0; c < 3; ++c) ad[A_JR + c] += rootv[12 + c] + ad[A_G + 9 + c] + rootv[9 + c];
    }
    wave_sync();
    // ---- rest joints are affine in beta
    if (lane < 10) {
#pragma unroll 8
        for (int i = 0; i < 48; ++i) a_beta = fmaf(tb[JSD + i * 10 + lane], ad[A_JR + i], a_beta);
    }
    // ---- Rodrigues (axis-angle -> unit quaternion -> matrix), 16 joints on 16 lanes
    if (lane < 16) {
        const float ax = sc[S_POSE + 3 * lane], ay = sc[S_POSE + 3 * lane + 1], az = sc[S_POSE + 3 * lane + 2];
        const float px = ax + 1e-8f, py = ay + 1e-8f, pz = az + 1e-8f;
        const float angle = sqrtf(px * px + py * py + pz * pz);
        const float nx = ax / angle, ny = ay / angle, nz = az / angle;
        const float half = angle * 0.5f;
        const float cs = cosf(half), sn = sinf(half);
        const float w0 = cs, x0 = sn * nx, y0 = sn * ny, z0 = sn * nz;
        const float qn = sqrtf(w0 * w0 + x0 * x0 + y0 * y0 + z0 * z0);
        const float w = w0 / qn, x = x0 / qn, y = y0 / qn, z = z0 / qn;
        const float *A = ad + A_ROT + 9 * lane;
        const float A0 = A[0], A1 = A[1], A2 = A[2], A3 = A[3], A4 = A[4], A5 = A[5], A6 = A[6], A7 = A[7], A8 = A[8];
        const float aw = 2.f * (w * (A0 + A4 + A8) + (-z * A1 + y * A2 + z * A3 - x * A5 - y * A6 + x * A7));
        const float axq = 2.f * (x * (A0 - A4 - A8) + (y * A1 + z * A2 + y * A3 - w * A5 + z * A6 + w * A7));
        const float ayq = 2.f * (y * (-A0 + A4 - A8) + (x * A1 + w * A2 + x * A3 + z * A5 - w * A6 + z * A7));
        const float azq = 2.f * (z * (-A0 - A4 + A8) + (-w * A1 + x * A2 + w * A3 + y * A5 + x * A6 + y * A7));
        const float qa = w * aw + x * axq + y * ayq + z * azq;
        const float bw = (aw - w * qa) / qn, bx = (axq - x * qa) / qn, by = (ayq - y * qa) / qn, bz = (azq - z * qa) / qn;
        const float a_sn = bx * nx + by * ny + bz * nz;
        const float anx = sn * bx, any_ = sn * by, anz = sn * bz;
        const float a_half = -sn * bw + cs * a_sn;
        const float a_angle = 0.5f * a_half - (anx * ax + any_ * ay + anz * az) / (angle * angle);
        ad[A_POSE + 3 * lane] = anx / angle + a_angle * px / angle;
        ad[A_POSE + 3 * lane + 1] = any_ / angle + a_angle * py / angle;
        ad[A_POSE + 3 * lane + 2] = anz / angle + a_angle * pz / angle;
    }
    wave_sync();
    return a_beta;
}

// d/d th45 of the 45 PCA-driven axis-angles' adjoints ad[A_POSE + 3 ..] (lane < 45; the last lanes repeat lane 44)
__device__ __forceinline__ float pca_bwd(const float *tb, const float *ad, int lane) {
    const int lc = lane < 45 ? lane : 44;
    float a45 = 0.f;
#pragma unroll 9
    for (int l = 0; l < 45; ++l) a45 = fmaf(tb[COMPS + lc * 45 + l], ad[A_POSE + 3 + l], a45);
    return a45;
}

// MODS: the likelihoods in log_p (MODS_UV and / or MODS_XYZ, as in mano_joints16_kernel)
// CHAM: log_p also carries -chamfer_w * (hand-object Chamfer distance of the row's joints, ch as in the loss pass; ch.dist is not used).  The
// wave finds the argmins again by the scan of the loss pass - no xyz or index tensor exists between the two passes - and the adjoint
// of the joints joins a_xyz.  LDS: none of its own (the joints a_j sit in the adjoint scratch, which is written only later).
template <int MODS, bool CHAM = false>
__global__ __launch_bounds__(256) void mano_joints_bwd_kernel(
    const float *__restrict__ th45_g, const float *__restrict__ det_g, const float *__restrict__ crop_uv,
    const float *__restrict__ vis, const float *__restrict__ pose3d, const float *__restrict__ tables, const float *__restrict__ g_logp,
    float *__restrict__ g_th45_o, float *__restrict__ g_det_o, int R, int B, float lap_b, float lap_b3, float th45_alpha, float row_w,
    ChamferArgs ch, float chamfer_w) {
    static_assert(MODS >= 1 && MODS <= 3, "mano_joints_bwd_kernel instantiation");
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float *tb = smem;
    for (int i = threadIdx.x; i < JOINT_FLOATS / 4; i += 256)
        reinterpret_cast<float4 *>(tb)[i] = reinterpret_cast<const float4 *>(tables)[i];
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    float *sc = smem + JOINT_FLOATS + wave * SCRATCH;
    float *ad = smem + JOINT_FLOATS + 4 * SCRATCH + wave * A_SCRATCH;

    for (int r = blockIdx.x * 4 + wave; r < R; r += gridDim.x * 4) {
        const int b = r % B;
        const float th45 = lane < 45 ? th45_g[(size_t)r * 45 + lane] : 0.f;
        const float det = lane < 16 ? det_g[b * 16 + lane] : 0.f;
        const RowOut o = joint_pass(tb, sc, lane, th45, det);
        const float g = g_logp[b] * row_w;                 // d loss / d log_p of this row
        const int c3 = lane % 3, k21 = lane < 63 ? lane / 3 : 20;

        // ---- Laplace on the projected joints and the projection itself
        const float s_cam = expf(bcast(det, 13));
        const float t_cam = (lane & 1) ? bcast(det, 15) : bcast(det, 14);
        const int lu = lane < 42 ? lane : 41;
        const float uv = s_cam * __shfl(o.xyz, 3 * (lu >> 1) + (lu & 1), 64) + t_cam;
        float a_uv = 0.f;
        if ((MODS & MODS_UV) && lane < 42) {
            const float d = uv - crop_uv[b * 42 + lane];
            if (vis[b * 21 + (lane >> 1)] == 1.f && fabsf(d) > 1e-4f) a_uv = (d > 0.f ? -g : g) / lap_b;
        }
        const float a_logs = wave_sum(a_uv * (uv - t_cam));
        const float a_t0 = wave_sum((lane & 1) ? 0.f : a_uv);
        const float a_t1 = wave_sum((lane & 1) ? a_uv : 0.f);
        const float a_uv_j = __shfl(a_uv, 2 * k21 + (c3 < 2 ? c3 : 0), 64);
        float a_xyz = (lane < 63 && c3 < 2) ? s_cam * a_uv_j : 0.f;
        if constexpr ((MODS & MODS_XYZ) != 0) {
            // ---- Laplace on the normalised joints (hand/network.py:620-643).  The root's normalised coordinates are identically 0:
            // their terms are constant and take no adjoint (the Sc cancellation below would only leave round-off of it)
            if (lane < 63 && k21 != kRootIdx) {
                const float d = o.xyz - pose3d[b * 63 + lane];
                if (vis[b * 21 + k21] == 1.f && fabsf(d) > 1e-4f) a_xyz += (d > 0.f ? -g : g) / lap_b3;
            }
        }
        if constexpr (CHAM) {
            // ---- dist = mean_j min_v |a_j - o_v| + mean_v min_j |a_j - o_v|,  a_j = xyz_j (scale[b] 1000) + root[b]  (hand/criteria.py:18-39)
            // d|a - o| / da = (a - o) / |a - o|, 0 at a zero distance (as chamfer_bwd_kernel); argmins fixed, ties to the lowest index
            const float su = ch.scale[b] * kChamferUnit;
            if (lane < 63) ad[lane] = fmaf(o.xyz, su, ch.root[(size_t)b * 3 + c3]);
            wave_sync();
            const int Vb = ch.obj_count ? min(max(ch.obj_count[b], 1), ch.VO) : ch.VO;
            const float *ob = ch.obj + (size_t)b * ch.VO * 3;
            float m1[21];
            int i1[21];
#pragma unroll
            for (int j = 0; j < 21; ++j) { m1[j] = __builtin_inff(); i1[j] = 0; }
            float acc = 0.f;        // lane 3 j + c: component c of sum over the vertices nearest to joint j of their unit vectors
            for (int t0 = 0; t0 < Vb; t0 += 64) {
                // lanes stride over the vertices: 64 per round, lane = vertex t0 + lane (past V_b: the last one again, taking part in nothing)
                const int v = t0 + lane;
                const bool ok = v < Vb;
                const size_t vo = (size_t)(ok ? v : Vb - 1) * 3;
                const float ox = ob[vo], oy = ob[vo + 1], oz = ob[vo + 2];
                float m2 = __builtin_inff();
                int j2 = 0;
#pragma unroll
                for (int j = 0; j < 21; ++j) {
                    const float d = chamfer_sqdist(ad[3 * j], ad[3 * j + 1], ad[3 * j + 2], ox, oy, oz);
                    if (ok && d < m1[j]) { m1[j] = d; i1[j] = v; }
                    if (d < m2) { m2 = d; j2 = j; }
                }
                float ux = 0.f, uy = 0.f, uz = 0.f;
                if (ok && m2 > 0.f) {
                    const float inv = 1.f / sqrtf(m2);
                    ux = (ad[3 * j2] - ox) * inv; uy = (ad[3 * j2 + 1] - oy) * inv; uz = (ad[3 * j2 + 2] - oz) * inv;
                }
                if (!ok) j2 = -1;
                // object -> hand scatter in a fixed order, no atomics: one masked wave reduction per joint that some vertex of the round chose
                for (int j = 0; j < 21; ++j) {
                    const bool mine = j2 == j;
                    if (__any(mine)) {
                        const float sx = wave_sum(mine ? ux : 0.f), sy = wave_sum(mine ? uy : 0.f), sz = wave_sum(mine ? uz : 0.f);
                        if (k21 == j) acc += c3 == 0 ? sx : (c3 == 1 ? sy : sz);
                    }
                }
            }
            // hand -> object: the lanes' (minimum, vertex) pairs to the wave's, the lower vertex on equal minima
            int iv = 0;
#pragma unroll
            for (int j = 0; j < 21; ++j) {
                float m = m1[j];
                int i = i1[j];
#pragma unroll
                for (int of = 32; of > 0; of >>= 1) {
                    const float om = __shfl_xor(m, of, 64);
                    const int oi = __shfl_xor(i, of, 64);
                    if (om < m || (om == m && oi < i)) { m = om; i = oi; }
                }
                if (k21 == j) iv = i;
            }
            float u1 = 0.f;
            {
                const size_t vo = (size_t)iv * 3;         // iv < V_b: an index some lane scanned (0 where a lane scanned none)
                const float dx = ad[3 * k21] - ob[vo], dy = ad[3 * k21 + 1] - ob[vo + 1], dz = ad[3 * k21 + 2] - ob[vo + 2];
                const float q = fmaf(dz, dz, fmaf(dy, dy, dx * dx));
                if (q > 0.f) u1 = (c3 == 0 ? dx : (c3 == 1 ? dy : dz)) * (1.f / sqrtf(q));
            }
            // the root's normalised coordinates are identically 0 (a constant a_12 = root[b]): it takes part in both minima, no adjoint
            if (lane < 63 && k21 != kRootIdx) a_xyz += (-chamfer_w * g * su) * fmaf(u1, 1.f / 21.f, acc * (1.f / (float)Vb));
            wave_sync();            // the adjoint scratch is written from here on
        }

        // ---- xyz = (J - J_root) / |J_norm - J_root|
        const float L = o.bone;
        const float S0 = wave_sum(c3 == 0 ? a_xyz : 0.f), S1 = wave_sum(c3 == 1 ? a_xyz : 0.f), S2 = wave_sum(c3 == 2 ? a_xyz : 0.f);
        const float Sc = c3 == 0 ? S0 : (c3 == 1 ? S1 : S2);
        const float a_L = -wave_sum(lane < 63 ? a_xyz * o.xyz : 0.f) / L;
        const float dc = sc[S_J21 + 3 * kNormIdx + c3] - sc[S_J21 + 3 * kRootIdx + c3];
        float aJ = a_xyz / L;
        if (k21 == kNormIdx) aJ += a_L * dc / L;
        if (k21 == kRootIdx) aJ -= Sc / L + a_L * dc / L;
        // ---- undo the reorder and the metre -> mm scale; the centring joint receives sum_k aJ = 0
        if (lane < 63) ad[A_PRE + 3 * kJointReorder[kFreihand2Rhd[k21]] + c3] = 1000.f * aJ;
        wave_sync();

        // ---- fingertip skinning, blend shapes of the tips, kinematic chain, Rodrigues
        const float a_beta = joint_chain_bwd<false>(tb, sc, ad, lane, nullptr);
        // ---- PCA coefficients and the soft priors
        {
            float a45 = pca_bwd(tb, ad, lane);
            const float v45 = fmaxf(fabsf(th45) / 2.f - 1.f, 0.f);
            a45 -= g * th45_alpha * v45 * (th45 > 0.f ? 1.f : -1.f);        // d/dx -alpha relu(|x|/2-1)^2
            if (lane < 45) g_th45_o[(size_t)r * 45 + lane] = a45;
        }
        {
            const float d0 = bcast(det, 0), d1 = bcast(det, 1), d2 = bcast(det, 2);
            const float r3 = sqrtf(d0 * d0 + d1 * d1 + d2 * d2);
            const float v3 = fmaxf(r3 / 3.14159265358979323846f - 1.f, 0.f);
            const float ab = __shfl(a_beta, lane >= 3 && lane < 13 ? lane - 3 : 0, 64);
            float out = 0.f;
            if (lane < 3) out = ad[A_POSE + lane] - (v3 > 0.f ? g * 10.f * v3 / 3.14159265358979323846f * det / r3 : 0.f);
            else if (lane < 13) {
                const float vb = fmaxf(fabsf(det) / 0.03f - 1.f, 0.f);
                out = ab - g * 100.f * vb / 0.03f * (det > 0.f ? 1.f : -1.f);
            } else if (lane == 13) out = a_logs;
            else if (lane == 14) out = a_t0;
            else if (lane == 15) out = a_t1;
            if (lane < 16) g_det_o[(size_t)r * 16 + lane] = out;
        }
        wave_sync();
    }
}

// Reverse of the full mesh's pose pass (mano_pose_kernel -> the skinning kernels): one wavefront per hypothesis re-runs joint_pass, seeds the
// adjoint scratch from the row's adjoint record of the skinning reverse (mano_skin_bwd.hip: g_pm | g_beta | g_G | g_centre, g_root, g_bone in
// the workspace row's layout) and walks joint_chain_bwd.  g_centre lands on the centring joint (pre-reorder joint kCenterPre, metres), g_root
// and g_bone on final joints kRootIdx / kNormIdx (mm, centred, RHD order; in mm_mode the record holds zeros there), g_joints_mm [R,63] - the
// adjoint of the joints_mm output, or NULL - on the final joints as well.  g_z [R,61] in z's column order (th3, th45, beta, log s, t); the
// camera columns 58..60 do not reach the mesh and are written as 0.
__global__ __launch_bounds__(256) void mano_verts_bwd_kernel(const float *__restrict__ z_g, const float *__restrict__ tables,
                                                             const float *__restrict__ adj, const float *__restrict__ g_joints_mm,
                                                             float *__restrict__ g_z, int R) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float *tb = smem;
    for (int i = threadIdx.x; i < JOINT_FLOATS / 4; i += 256)
        reinterpret_cast<float4 *>(tb)[i] = reinterpret_cast<const float4 *>(tables)[i];
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    float *sc = smem + JOINT_FLOATS + wave * SCRATCH;
    float *ad = smem + JOINT_FLOATS + 4 * SCRATCH + wave * A_SCRATCH;
    for (int r = blockIdx.x * 4 + wave; r < R; r += gridDim.x * 4) {
        const float *zr = z_g + (size_t)r * 61;
        const float th45 = lane < 45 ? zr[3 + lane] : 0.f;
        const float det = lane < 3 ? zr[lane] : (lane < 16 ? zr[45 + lane] : 0.f);      // as mano_pose_kernel
        const RowOut o = joint_pass(tb, sc, lane, th45, det);
        const float *ar = adj + (size_t)r * WS_STRIDE;
        const int c3 = lane % 3, k21 = lane < 63 ? lane / 3 : 20;
        // ---- adjoints of the final joints: root = J_12, bone = |J_11 - J_12|
        float aJ = (g_joints_mm && lane < 63) ? g_joints_mm[(size_t)r * 63 + lane] : 0.f;
        const float dc = sc[S_J21 + 3 * kNormIdx + c3] - sc[S_J21 + 3 * kRootIdx + c3];
        const float a_dc = ar[WS_NRM + 6] * dc / o.bone;
        if (lane < 63 && k21 == kNormIdx) aJ += a_dc;
        if (lane < 63 && k21 == kRootIdx) aJ += ar[WS_NRM + 3 + c3] - a_dc;
        // ---- J_k = (pre[reorder(k)] - centre) 1000: the centring joint takes g_centre - 1000 sum_k aJ_k on top of its own
        const float S0 = wave_sum(c3 == 0 ? aJ : 0.f), S1 = wave_sum(c3 == 1 ? aJ : 0.f), S2 = wave_sum(c3 == 2 ? aJ : 0.f);
        if (lane < 63) ad[A_PRE + 3 * kJointReorder[kFreihand2Rhd[k21]] + c3] = 1000.f * aJ;
        wave_sync();
        if (lane < 3) ad[A_PRE + 3 * kCenterPre + lane] += ar[WS_NRM + lane] - 1000.f * (lane == 0 ? S0 : (lane == 1 ? S1 : S2));
        wave_sync();
        const float a_beta = joint_chain_bwd<true>(tb, sc, ad, lane, ar);
        const float a45 = pca_bwd(tb, ad, lane);
        float *gz = g_z + (size_t)r * 61;
        if (lane < 3) { gz[lane] = ad[A_POSE + lane]; gz[58 + lane] = 0.f; }
        if (lane < 45) gz[3 + lane] = a45;
        if (lane < 10) gz[48 + lane] = a_beta;
        wave_sync();
    }
}

// z is a gather of (det, th45) (mano_pose_kernel: th3 = det[0:3], th45, beta = det[3:13], (log s, t) = det[13:16]): the adjoint of z, with
// its camera columns taken from g_logs_t, is added to the two buffers the loss pass' reverse wrote.  One thread per column of a row, one add.
__global__ __launch_bounds__(256) void mano_z_grad_add_kernel(const float *__restrict__ g_z, const float *__restrict__ g_logs_t,
                                                              float *__restrict__ g_th45, float *__restrict__ g_det_rows, int R) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)R * 61) return;
    const size_t r = i / 61;
    const int c = (int)(i - r * 61);
    if (c >= 58) {
        if (g_logs_t) g_det_rows[r * 16 + 13 + (c - 58)] += g_logs_t[r * 3 + (c - 58)];
        return;
    }
    const float g = g_z[i];
    if (c < 3) g_det_rows[r * 16 + c] += g;
    else if (c < 48) g_th45[r * 45 + (c - 3)] += g;
    else g_det_rows[r * 16 + 3 + (c - 48)] += g;
}

// transpose of regress_joints_kernel (mano.hip): g_verts[v] (+)=sum_j J_regressor[j][v] g_kp[map(j)] + g_kp[tip] at the five tip vertices,
// g_kp = g_joints with the RHD reorder undone.  One workgroup per hypothesis, one thread per vertex: a fixed-order sum, no atomics
__global__ __launch_bounds__(256) void regress_joints_bwd_kernel(const float *__restrict__ g_joints, const float *__restrict__ tables,
                                                                 float *__restrict__ g_verts, int R, int accumulate) {
    __shared__ float gk[21 * 3];
    const int r = blockIdx.x;
    if (threadIdx.x < 63) gk[3 * kFreihand2Rhd[threadIdx.x / 3] + threadIdx.x % 3] = g_joints[(size_t)r * 63 + threadIdx.x];
    __syncthreads();
    float *o = g_verts + (size_t)r * NV * 3;
    for (int v = threadIdx.x; v < NV; v += 256) {
        float a0 = 0.f, a1 = 0.f, a2 = 0.f;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const float w = tables[V_JR + j * VP + v];
            const float *g = gk + 3 * kWrapJointMap[j];
            a0 = fmaf(w, g[0], a0); a1 = fmaf(w, g[1], a1); a2 = fmaf(w, g[2], a2);
        }
#pragma unroll
        for (int t = 0; t < 5; ++t)
            if (v == kWrapTipVert[t]) { a0 += gk[3 * (4 + 4 * t)]; a1 += gk[3 * (4 + 4 * t) + 1]; a2 += gk[3 * (4 + 4 * t) + 2]; }
        if (accumulate) { a0 += o[3 * v]; a1 += o[3 * v + 1]; a2 += o[3 * v + 2]; }
        o[3 * v] = a0; o[3 * v + 1] = a1; o[3 * v + 2] = a2;
    }
}

// out[b][c] = sum_n in[(n*B + b)][c]: per-image totals of per-hypothesis rows (det head and conditioning gradients)
__global__ __launch_bounds__(256) void sum_over_hypotheses_kernel(const float *__restrict__ in, float *__restrict__ out,
                                                                  int N, int B, int C, int accumulate, long out_stride) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)B * C) return;
    float acc = 0.f;
    for (int n = 0; n < N; ++n) acc += in[(size_t)n * B * C + i];
    float *o = out + (i / C) * out_stride + i % C;
    *o = accumulate ? *o + acc : acc;
}
}}  // namespace mhe::mano

using namespace mhe;

static int joints_bwd_launch(const char *who, const float *th45, const float *det, const float *crop_uv, const float *vis, const float *pose3d,
                             const float *tables, const float *g_log_p, float *g_th45, float *g_det_rows, int R, int B, int mods,
                             float laplace_b, float laplace_b_3d, float th45_alpha, float row_weight, void *stream,
                             const mano::ChamferArgs *ch = nullptr, float chamfer_w = 0.f) {
    MHE_REQUIRE(th45 && det && vis && tables && g_log_p && g_th45 && g_det_rows, "%s: null pointer", who);
    MHE_REQUIRE(mods >= 1 && mods <= (MHE_MODS_UV | MHE_MODS_XYZ), "%s: mods=%d must be a non-empty set of MHE_MODS_UV | MHE_MODS_XYZ", who, mods);
    MHE_REQUIRE(!(mods & MHE_MODS_UV) || crop_uv, "%s: mods has MHE_MODS_UV but crop_uv is null", who);
    MHE_REQUIRE(!(mods & MHE_MODS_XYZ) || pose3d, "%s: mods has MHE_MODS_XYZ but pose3d is null", who);
    MHE_REQUIRE(R > 0 && B > 0 && R % B == 0, "%s: R=%d must be a positive multiple of B=%d", who, R, B);
    MHE_REQUIRE(!(mods & MHE_MODS_UV) || laplace_b > 0.f, "%s: laplace_b must be > 0", who);
    MHE_REQUIRE(!(mods & MHE_MODS_XYZ) || laplace_b_3d > 0.f, "%s: laplace_b_3d must be > 0", who);
    const int blocks = (R + 3) / 4 < 2048 ? (R + 3) / 4 : 2048;
    const size_t lds = (mano::JOINT_FLOATS + 4 * (mano::SCRATCH + mano::A_SCRATCH)) * sizeof(float);
    if (ch) {
        auto kc = mods == MHE_MODS_UV ? mano::mano_joints_bwd_kernel<mano::MODS_UV, true>
                                      : (mods == MHE_MODS_XYZ ? mano::mano_joints_bwd_kernel<mano::MODS_XYZ, true>
                                                              : mano::mano_joints_bwd_kernel<mano::MODS_UV | mano::MODS_XYZ, true>);
        hipLaunchKernelGGL(kc, dim3(blocks), dim3(256), lds, (hipStream_t)stream, th45, det, crop_uv, vis, pose3d, tables, g_log_p, g_th45,
                           g_det_rows, R, B, laplace_b, laplace_b_3d, th45_alpha, row_weight, *ch, chamfer_w);
        return check_launch("mano_joints_bwd_kernel (chamfer)");
    }
    auto kern = mods == MHE_MODS_UV ? mano::mano_joints_bwd_kernel<mano::MODS_UV>
                                    : (mods == MHE_MODS_XYZ ? mano::mano_joints_bwd_kernel<mano::MODS_XYZ>
                                                            : mano::mano_joints_bwd_kernel<mano::MODS_UV | mano::MODS_XYZ>);
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(256), lds, (hipStream_t)stream, th45, det, crop_uv, vis, pose3d, tables, g_log_p, g_th45,
                       g_det_rows, R, B, laplace_b, laplace_b_3d, th45_alpha, row_weight, mano::ChamferArgs{}, 0.f);
    return check_launch("mano_joints_bwd_kernel");
}

extern "C" int mhe_mano_joints_bwd_f32(const float *th45, const float *det, const float *crop_uv, const float *vis,
                                       const float *tables, const float *g_log_p, float *g_th45, float *g_det_rows,
                                       int R, int B, float laplace_b, float th45_alpha, float row_weight, void *stream) {
    return joints_bwd_launch("mhe_mano_joints_bwd_f32", th45, det, crop_uv, vis, nullptr, tables, g_log_p, g_th45, g_det_rows, R, B,
                             MHE_MODS_UV, laplace_b, 0.f, th45_alpha, row_weight, stream);
}

extern "C" int mhe_mano_joints_mods_bwd_f32(const float *th45, const float *det, const float *crop_uv, const float *vis, const float *pose3d,
                                            const float *tables, const float *g_log_p, float *g_th45, float *g_det_rows, int R, int B,
                                            int mods, float laplace_b, float laplace_b_3d, float th45_alpha, float row_weight, void *stream) {
    return joints_bwd_launch("mhe_mano_joints_mods_bwd_f32", th45, det, crop_uv, vis, pose3d, tables, g_log_p, g_th45, g_det_rows, R, B,
                             mods, laplace_b, laplace_b_3d, th45_alpha, row_weight, stream);
}

// Reverse of mhe_mano_joints_chamfer_f32's  log_p[r] - chamfer_w dist[r]
extern "C" int mhe_mano_joints_chamfer_bwd_f32(const float *th45, const float *det, const float *crop_uv, const float *vis, const float *pose3d,
                                               const float *tables, const float *scale, const float *root, const float *obj, const int *obj_count,
                                               const float *g_log_p, float *g_th45, float *g_det_rows, int R, int B, int VO, int mods,
                                               float laplace_b, float laplace_b_3d, float th45_alpha, float row_weight, float chamfer_w,
                                               void *stream) {
    const char *who = "mhe_mano_joints_chamfer_bwd_f32";
    MHE_REQUIRE(scale && root && obj, "%s: null pointer (scale, root, obj)", who);
    MHE_REQUIRE(VO >= 1, "%s: VO=%d (VO >= 1)", who, VO);
    MHE_REQUIRE(chamfer_w == chamfer_w, "%s: chamfer_w is NaN", who);
    const mano::ChamferArgs ch{scale, root, obj, obj_count, nullptr, VO};
    return joints_bwd_launch(who, th45, det, crop_uv, vis, pose3d, tables, g_log_p, g_th45, g_det_rows, R, B, mods, laplace_b, laplace_b_3d,
                             th45_alpha, row_weight, stream, &ch, chamfer_w);
}

int mhe_mano_pose_rows(const float *z, const float *tables, float *rows, int R, hipStream_t stream);                      // mano.hip
size_t mhe_mano_skin_bwd_table_floats();                                                                                  // mano_skin_bwd.hip
int mhe_mano_skin_bwd(const float *ws_rows, const float *tables, float *bt, const float *g_verts, float *adj, int R, int mm_mode,
                      hipStream_t stream);

// workspace: the reverse's coefficient-fastest tables | the forward's workspace rows [R][352] | the adjoint rows [R][352]
extern "C" size_t mhe_mano_verts_bwd_workspace_floats(int R) {
    return R > 0 ? mhe_mano_skin_bwd_table_floats() + (size_t)2 * R * mano::WS_STRIDE : 0;
}

extern "C" int mhe_mano_verts_bwd_f32(const float *z, const float *tables, const float *g_verts, const float *g_joints_mm, float *g_z,
                                      float *workspace, int R, int mm_mode, void *stream) {
    const char *who = "mhe_mano_verts_bwd_f32";
    MHE_REQUIRE(z && tables && g_verts && g_z && workspace, "%s: null pointer", who);
    MHE_REQUIRE(R > 0, "%s: R=%d", who, R);
    const size_t nz = (size_t)R * 61 * 4, nt = (size_t)mano::TOTAL_FLOATS * 4, nv = (size_t)R * mano::NV * 12, nj = (size_t)R * 63 * 4,
                 nw = mhe_mano_verts_bwd_workspace_floats(R) * 4;
    MHE_REQUIRE(disjoint(g_z, nz, z, nz) && disjoint(g_z, nz, tables, nt) && disjoint(g_z, nz, g_verts, nv) && disjoint(g_z, nz, g_joints_mm, nj) &&
                    disjoint(workspace, nw, z, nz) && disjoint(workspace, nw, tables, nt) && disjoint(workspace, nw, g_verts, nv) &&
                    disjoint(workspace, nw, g_joints_mm, nj) && disjoint(workspace, nw, g_z, nz),
                "%s: g_z and workspace must not overlap the inputs or each other", who);
    const hipStream_t st = (hipStream_t)stream;
    float *rows = workspace + mhe_mano_skin_bwd_table_floats(), *adj = rows + (size_t)R * mano::WS_STRIDE;
    if (int rc = mhe_mano_pose_rows(z, tables, rows, R, st)) return rc;
    if (int rc = mhe_mano_skin_bwd(rows, tables, workspace, g_verts, adj, R, mm_mode, st)) return rc;
    const int blocks = (R + 3) / 4 < 2048 ? (R + 3) / 4 : 2048;
    const size_t lds = (mano::JOINT_FLOATS + 4 * (mano::SCRATCH + mano::A_SCRATCH)) * sizeof(float);
    hipLaunchKernelGGL(mano::mano_verts_bwd_kernel, dim3(blocks), dim3(256), lds, st, z, tables, adj, g_joints_mm, g_z, R);
    return check_launch("mano_verts_bwd_kernel");
}

extern "C" int mhe_mano_z_grad_add_f32(const float *g_z, const float *g_logs_t, float *g_th45, float *g_det_rows, int R, void *stream) {
    const char *who = "mhe_mano_z_grad_add_f32";
    MHE_REQUIRE(g_z && g_th45 && g_det_rows, "%s: null pointer (g_z, g_th45, g_det_rows)", who);
    MHE_REQUIRE(R > 0, "%s: R=%d", who, R);
    const size_t nz = (size_t)R * 61 * 4, nl = (size_t)R * 12, n45 = (size_t)R * 45 * 4, nd = (size_t)R * 16 * 4;
    MHE_REQUIRE(disjoint(g_th45, n45, g_z, nz) && disjoint(g_th45, n45, g_logs_t, nl) && disjoint(g_det_rows, nd, g_z, nz) &&
                    disjoint(g_det_rows, nd, g_logs_t, nl) && disjoint(g_th45, n45, g_det_rows, nd),
                "%s: g_th45 and g_det_rows must not overlap the inputs or each other", who);
    const size_t n = (size_t)R * 61;
    hipLaunchKernelGGL(mano::mano_z_grad_add_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, g_z, g_logs_t, g_th45,
                       g_det_rows, R);
    return check_launch("mano_z_grad_add_kernel");
}

extern "C" int mhe_mano_regress_joints_bwd_f32(const float *g_joints, const float *tables, float *g_verts, int R, int accumulate, void *stream) {
    const char *who = "mhe_mano_regress_joints_bwd_f32";
    MHE_REQUIRE(g_joints && tables && g_verts, "%s: null pointer", who);
    MHE_REQUIRE(R > 0, "%s: R=%d", who, R);
    const size_t nv = (size_t)R * mano::NV * 12;
    MHE_REQUIRE(disjoint(g_verts, nv, g_joints, (size_t)R * 63 * 4) && disjoint(g_verts, nv, tables, (size_t)mano::TOTAL_FLOATS * 4),
                "%s: g_verts must not overlap the inputs", who);
    hipLaunchKernelGGL(mano::regress_joints_bwd_kernel, dim3(R), dim3(256), 0, (hipStream_t)stream, g_joints, tables, g_verts, R, accumulate);
    return check_launch("regress_joints_bwd_kernel");
}

extern "C" int mhe_sum_over_hypotheses_f32(const float *rows, float *out, int N, int B, int C, int accumulate, long out_stride,
                                           void *stream) {
    MHE_REQUIRE(rows && out && N > 0 && B > 0 && C > 0, "mhe_sum_over_hypotheses_f32: bad arguments");
    if (out_stride <= 0) out_stride = C;
    MHE_REQUIRE(out_stride >= C, "mhe_sum_over_hypotheses_f32: out_stride=%ld < C=%d", out_stride, C);
    const size_t n = (size_t)B * C;
    hipLaunchKernelGGL(mano::sum_over_hypotheses_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       rows, out, N, B, C, accumulate, out_stride);
    return check_launch("sum_over_hypotheses_kernel");
}
