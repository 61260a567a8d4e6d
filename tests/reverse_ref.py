"""Float64 CPU references of the reverse pass's small kernels (csrc/trunk_bwd.hip, csrc/flow_bwd.hip), one per operation, written from the
kernels' comments and the mathematics.  A helper module, not a test: tests/test_reverse_ref_host.py checks every reference against float64
torch autograd of the operation it differentiates, tests/test_gpu_reverse_edges.py checks the kernels against the references.

Every function takes CPU tensors holding the values the kernel reads (already rounded to the storage type), computes in float64 and returns
the expected value together with the magnitude its error bound is stated in (the sum of the magnitudes of the partial results).  Activations
are channels-last: [..., C] with per-channel tables [C]."""
import numpy as np
import torch

F64 = torch.float64


def d(t):
    return None if t is None else torch.as_tensor(t).to(F64)


def stored(t, dt):
    """the f64 values a tensor of storage type dt would hold of t (round to nearest even through f32, as the kernels' stores do)"""
    return t.to(torch.float32).to(dt).to(F64)


# ---- BatchNorm (train mode) reverse --------------------------------------------------------------------------------------------------------
def gated(g, a):
    """g' = g [a > 0] (the ReLU behind the BatchNorm; a = None: no gate)"""
    g = d(g)
    return g if a is None else torch.where(d(a) > 0, g, torch.zeros_like(g))


def bn_bwd_sums(g, a, y, mean, invstd):
    """per-channel (sum g', sum g' xhat, sum |g'|, sum |g' xhat|) over all leading dimensions, xhat = (y - mean) invstd"""
    gp = gated(g, a).reshape(-1, g.shape[-1])
    t = gp * ((d(y).reshape(gp.shape) - d(mean)) * d(invstd))
    return gp.sum(0), t.sum(0), gp.abs().sum(0), t.abs().sum(0)


def bn_bwd_coef(s1, s2, gamma, mean, invstd, count):
    """dbeta = s1, dgamma = s2 and the coefficients of gy = k2 g' + k1 y + k0 = gamma invstd (g' - dbeta / M - xhat dgamma / M);
    k0mag = |k2 dbeta / M| + |k1 mean|, the magnitude k0's bound is stated in"""
    s1, s2, gamma, mean, invstd = d(s1), d(s2), d(gamma), d(mean), d(invstd)
    k2 = gamma * invstd
    k1 = -k2 * invstd * s2 / count
    k0 = -k2 * s1 / count - k1 * mean
    return {"dbeta": s1, "dgamma": s2, "k2": k2, "k1": k1, "k0": k0, "k0mag": (k2 * s1 / count).abs() + (k1 * mean).abs()}


def bn_bwd_apply(g, a, y, k2, k1, k0):
    """(gy, |k2 g'| + |k1 y| + |k0|, g')"""
    gp, y, k2, k1, k0 = gated(g, a), d(y), d(k2), d(k1), d(k0)
    return k2 * gp + k1 * y + k0, (k2 * gp).abs() + (k1 * y).abs() + k0.abs(), gp


def mean_invstd(s1, s2, count, eps):
    """(mean, 1 / sqrt(var + eps)) of the forward's sums s1 = sum y, s2 = sum y^2 (biased variance, clamped at 0)"""
    mean = d(s1) / count
    var = (d(s2) / count - mean * mean).clamp_min(0.0)
    return mean, 1.0 / torch.sqrt(var + eps)


def bn_backward(g, a, y, gamma, eps):
    """the whole reverse from the activations alone (batch statistics of y): (gy, dgamma, dbeta)"""
    y2 = d(y).reshape(-1, y.shape[-1])
    M = y2.shape[0]
    mean, istd = mean_invstd(y2.sum(0), (y2 * y2).sum(0), M, eps)
    s1, s2, _, _ = bn_bwd_sums(g, a, y, mean, istd)
    c = bn_bwd_coef(s1, s2, gamma, mean, istd, M)
    return bn_bwd_apply(g, a, y, c["k2"], c["k1"], c["k0"])[0], c["dgamma"], c["dbeta"]


# ---- 3x3 / stride-2 / pad-1 max pool with winners ------------------------------------------------------------------------------------------
def pooled_size(H, W):
    return (H - 1) // 2 + 1, (W - 1) // 2 + 1


def _taps(x):
    """for tap = dh * 3 + dw: (values [B, Ho, Wo, C] at input pixel (2 ho - 1 + dh, 2 wo - 1 + dw), clamped into the image; valid [Ho, Wo])"""
    B, H, W, C = x.shape
    Ho, Wo = pooled_size(H, W)
    ho, wo = torch.arange(Ho), torch.arange(Wo)
    for dh in range(3):
        for dw in range(3):
            hi, wi = 2 * ho - 1 + dh, 2 * wo - 1 + dw
            ok = ((hi >= 0) & (hi < H))[:, None] & ((wi >= 0) & (wi < W))[None, :]
            yield dh * 3 + dw, x[:, hi.clamp(0, H - 1)][:, :, wi.clamp(0, W - 1)], ok


def maxpool_winners(x):
    """(pooled, tap uint8) of NHWC x in its own type: the first maximum in scan order over the taps inside the image, starting from the first
    such tap (so a window of -inf pools to -inf at a real pixel; the centre tap is always inside); a NaN wins over every number and stays
    (torch's max_pool2d rule)"""
    m = tap = None
    for j, v, ok in _taps(x):
        ok = ok[None, :, :, None].expand(v.shape)
        if m is None:
            m, tap = torch.zeros_like(v), torch.full(v.shape, 255, dtype=torch.uint8)
        win = ok & ((tap == 255) | (v > m) | (torch.isnan(v) & ~torch.isnan(m)))
        m, tap = torch.where(win, v, m), torch.where(win, torch.full_like(tap, j), tap)
    return m, tap


def affine_relu(x, scale, shift, dt):
    """relu(x scale + shift) in f64, as a tensor of storage type dt would hold it (the values the fused pool compares and gates on)"""
    return stored((d(x) * d(scale) + d(shift)).clamp_min(0.0), dt)


def window_pixels(tap, H, W):
    """(hi, wi) int64 [B, Ho, Wo, C]: the input pixel each recorded tap names"""
    Ho, Wo = tap.shape[1], tap.shape[2]
    hi = 2 * torch.arange(Ho)[None, :, None, None] - 1 + (tap // 3).long()
    wi = 2 * torch.arange(Wo)[None, None, :, None] - 1 + (tap % 3).long()
    return hi, wi


def gather_winners(x, tap):
    """x at the winners [B, Ho, Wo, C]"""
    B, H, W, C = x.shape
    hi, wi = window_pixels(tap, H, W)
    bi = torch.arange(B)[:, None, None, None].expand_as(hi)
    ci = torch.arange(C)[None, None, None, :].expand_as(hi)
    return x[bi, hi, wi, ci]


def maxpool_bwd(gy, tap, H, W):
    """gx [B, H, W, C] f64: every pooled gradient added to the pixel its tap names"""
    B, Ho, Wo, C = gy.shape
    hi, wi = window_pixels(tap, H, W)
    bi = torch.arange(B)[:, None, None, None].expand_as(hi)
    ci = torch.arange(C)[None, None, None, :].expand_as(hi)
    flat = ((bi * H + hi) * W + wi) * C + ci
    return torch.zeros(B * H * W * C, dtype=F64).index_add_(0, flat.reshape(-1), d(gy).reshape(-1)).view(B, H, W, C)


def avgpool_bwd(g, HW, mask=None):
    """gx[b, p, c] = g[b, c] / HW [mask > 0]"""
    B, C = g.shape
    gx = (d(g) / HW)[:, None, :].expand(B, HW, C)
    return gx.clone() if mask is None else torch.where(d(mask).reshape(B, HW, C) > 0, gx, torch.zeros(()).to(F64))


def upsample2(g, H, W, base=None):
    """(out, |base| + |g placed|): out[b, 2i, 2j] = g[b, i, j] (+ base), 0 (+ base) elsewhere: the reverse of x[:, ::2, ::2]"""
    B, Ho, Wo, C = g.shape
    z = torch.zeros(B, H, W, C, dtype=F64)
    z[:, ::2, ::2] = d(g)
    if base is None:
        return z, z.abs()
    return z + d(base), z.abs() + d(base).abs()


# ---- gradient norm, clip + Adam ----------------------------------------------------------------------------------------------------------------
def sqnorm(g):
    return float((d(g) ** 2).sum())


def pow_abs_err(x):
    """one ulp of a float32 transcendental result x, or the smallest normal number where the result may be flushed"""
    return np.maximum(np.spacing(np.abs(np.asarray(x, np.float64)).astype(np.float32)).astype(np.float64), 2.0 ** -126)


def clip_adam(p, g, m, v, t, sq, lr, b1, b2, eps, max_norm, grad_scale, u=2.0 ** -24, k_pow=1.0, tiny=1e-6):
    """one step of clip_grad_norm_(max_norm) + Adam (no weight decay, no amsgrad) in f64, and the derived per-element error bounds:
      coef = grad_scale min(1, max_norm / (sqrt(sq) grad_scale + 1e-6));  g' = g coef;  m' = b1 m + (1 - b1) g';  v' = b2 v + (1 - b2) g'^2;
      p' = p - lr / (1 - b1^t) m' / (sqrt(v') / sqrt(1 - b2^t) + eps)
    sq = sum g^2 as the kernel reads it (None: no clipping).  Returns {p, m, v, bp, bm, bv}: the bounds follow the kernel's operation count
    (u per rounding, k_pow ulp per powf result), first order, each term against the magnitude of the partial result it rounds."""
    p, g, m, v = d(p), d(g), d(m), d(v)
    coef, e_coef = grad_scale, 0.0
    if max_norm > 0:
        cc = max_norm / (np.sqrt(sq) * grad_scale + tiny)
        coef, e_coef = grad_scale * min(1.0, cc), 5 * u          # sqrt, product, sum, division, product
    gg = g * coef
    e_g = e_coef + u                                             # relative error of g'
    m2 = b1 * m + (1 - b1) * gg
    bm = 2 * u * (b1 * m).abs() + (e_g + 3 * u) * ((1 - b1) * gg).abs()          # product + sum | 1 - b1, product, sum
    v2 = b2 * v + (1 - b2) * gg * gg
    bv = 2 * u * (b2 * v).abs() + (2 * e_g + 4 * u) * ((1 - b2) * gg * gg).abs()
    pw1, pw2 = b1 ** t, b2 ** t
    bc1, x2 = 1 - pw1, 1 - pw2
    e1 = (k_pow * float(pow_abs_err(pw1)) + u * bc1) / bc1                        # relative error of 1 - b1^t
    e2 = (k_pow * float(pow_abs_err(pw2)) + u * x2) / x2
    e_bc2 = e2 / 2 + u                                                            # of sqrt(1 - b2^t)
    step_size, bc2s = lr / bc1, np.sqrt(x2)
    root = torch.sqrt(v2)
    d_root = torch.sqrt(v2 + bv) - torch.sqrt((v2 - bv).clamp_min(0.0)) + u * root
    denom = root / bc2s + eps
    d_denom = d_root / bc2s + (root / bc2s) * (e_bc2 + u) + u * denom
    upd = step_size * m2 / denom
    d_upd = upd.abs() * (e1 + 3 * u + d_denom / denom) + (step_size / denom) * bm
    p2 = p - upd
    return {"p": p2, "m": m2, "v": v2, "bm": bm, "bv": bv, "bp": d_upd + u * (p.abs() + upd.abs())}


# ---- RealNVP stages ----------------------------------------------------------------------------------------------------------------------------
XP = 64          # padded width of the flow variable as a GEMM operand


def mask_pad(x, mask):
    """[R, 64]: x mask in the first dim columns, 0 in the padding"""
    R, dim = x.shape
    out = torch.zeros(R, XP, dtype=F64)
    out[:, :dim] = d(x) * d(mask)
    return out


def cond_lrelu(pre, cond, B, slope):
    """(leaky_relu(pre[r] + cond[r % B]), |pre| + |cond|)"""
    R = pre.shape[0]
    c = d(cond)[torch.arange(R) % B]
    t = d(pre) + c
    return torch.where(t > 0, t, slope * t), d(pre).abs() + c.abs()


def lrelu_bwd(g, h, slope):
    return torch.where(d(h) > 0, d(g), slope * d(g))


def coupling_forward(x, Os, Ot, mask):
    """one affine coupling: (x_out, log q increment) = (m x + (1 - m)(x e^s + t), - sum_d s), s = tanh(Os)(1 - m), t = Ot (1 - m);
    Os / Ot [R, dim]"""
    m = d(mask)
    s, t = torch.tanh(Os) * (1 - m), Ot * (1 - m)
    return m * x + (1 - m) * (x * torch.exp(s) + t), -s.sum(1)


def couple_bwd(x_out, Os, Ot, mask, g_out, g_logp, q_weight, B, u=2.0 ** -24, k=1.0):
    """the coupling's reverse from its output (binary mask): x_in = m x_out + (1 - m)(x_out - t) e^-s and, with a_q[r] = g_logp[r % B] q_weight
    the adjoint of log q,  GOs = (1 - m)(g_out x_in e^s - a_q)(1 - tanh^2 Os),  GOt = (1 - m) g_out,  g_part = g_out (m + (1 - m) e^s).
    Os / Ot [R, 64] (the first dim columns are read); GOs / GOt come back [R, 64] with +0 padding.  Bounds (first order): tanhf and expf
    contribute k ulp of their result, every other operation u of its result; 1 - s^2 carries the ABSOLUTE error 2 |s| ds + u."""
    R, dim = x_out.shape
    xo, go, m = d(x_out), d(g_out), d(mask)
    os_, ot = d(Os)[:, :dim], d(Ot)[:, :dim]
    on = (m == 0).expand(R, dim)
    ulp = lambda t: torch.as_tensor(np.spacing(t.abs().numpy().astype(np.float32)).astype(np.float64))
    s = torch.tanh(os_)
    ds = k * ulp(s)
    es = torch.exp(s)
    des = es * ds + k * ulp(es)
    xi = (xo - ot) / es
    dxi = xi.abs() * (2 * u + des / es)
    a_q = torch.zeros(R, 1, dtype=F64) if g_logp is None else (d(g_logp)[torch.arange(R) % B] * q_weight)[:, None]
    A = go * xi * es
    dA = A.abs() * (dxi / xi.abs().clamp_min(1e-300) + des / es + 2 * u)
    diff = A - a_q
    ddiff = dA + u * a_q.abs() + u * (A.abs() + a_q.abs())
    T = 1 - s * s
    dT = 2 * s.abs() * ds + u
    gos = diff * T
    dgos = diff.abs() * dT + T * ddiff + u * gos.abs()
    gp = go * es
    dgp = go.abs() * des + u * gp.abs()
    z = torch.zeros(R, dim, dtype=F64)
    pad = lambda t: torch.cat([t, torch.zeros(R, XP - dim, dtype=F64)], 1)
    return {"x_in": torch.where(on, xi, xo), "b_x_in": torch.where(on, dxi, z), "GOs": pad(torch.where(on, gos, z)),
            "b_GOs": pad(torch.where(on, dgos, z)), "GOt": pad(torch.where(on, go, z)), "g_part": torch.where(on, gp, go),
            "b_g_part": torch.where(on, dgp, z)}


def couple_accum(g_part, GXs, GXt, mask):
    """(g_part + m (GXs + GXt), |g_part| + |m| (|GXs| + |GXt|)); GXs / GXt [R, 64]"""
    dim = g_part.shape[1]
    a, b, m = d(GXs)[:, :dim], d(GXt)[:, :dim], d(mask)
    return d(g_part) + m * (a + b), d(g_part).abs() + m.abs() * (a.abs() + b.abs())
