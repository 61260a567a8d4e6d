"""Float64 CPU references of the conditional Glow's staged kernels (csrc/glow.hip) and of the dense layer they run on (mhe_linear_f32,
csrc/conv.hip), one per stage, written from the kernels' comments and oracle/glow_ref.py.  A helper module, not a test:
tests/test_glow_stage_ref_host.py checks every backward reference against float64 torch autograd of its forward reference (and the coupling /
finish references against oracle/glow_ref.py), tests/test_gpu_glow_edges.py checks the kernels against the references.

Every function takes CPU tensors holding the values the kernel reads (already rounded to the storage type, f32 or bf16) and computes in
float64.  Values travel as `V` pairs (value, first-order bound of the error a float32 evaluation in the kernel's operation order may
have): every operation adds u32 = 2^-24 of its result, expf / logf one ulp (2 u32) of theirs, and 2^-126 because a result below the
smallest normal float32 may come out as zero (that is what covers expf(104) = inf: 1 / (1 + inf) = 0 against a true 6.8e-46).  Sums
carry the length L of the longest serial chain: L u32 sum |term|.  Nothing here is fitted to a kernel."""
import numpy as np
import torch

F64 = torch.float64
U32, UB, TINY = 2.0 ** -24, 2.0 ** -8, 2.0 ** -126
C1E3 = float(np.float32(1e-3))                                # the kernels' own float32 constants
LOG2PI = float(np.float32(1.8378770664093453))


_DT = [F64]


def d(t):
    return None if t is None else torch.as_tensor(t).to(_DT[0])


class plain_float32:
    """inside this context every reference evaluates its formula in plain float32 torch on the CPU (the error fields mean nothing then): the
    evaluation whose distance from float64 sizes the margin for expf / logf in tests/test_gpu_glow_edges.py"""

    def __enter__(self):
        _DT[0] = torch.float32

    def __exit__(self, *exc):
        _DT[0] = F64
        return False


def stored(t, dt):
    """the f64 values a tensor of storage type dt would hold of t (round to nearest even through f32, as the kernels' stores do)"""
    return t.to(torch.float32).to(dt).to(F64)


class V:
    """a float64 value with the bound of its float32 evaluation error"""

    def __init__(self, v, e=None):
        self.v = d(v)
        self.e = torch.zeros_like(self.v) if e is None else e

    def __neg__(self):
        return V(-self.v, self.e)


def _v(x):
    return x if isinstance(x, V) else V(x)


def _r(v):
    return U32 * v.detach().abs() + TINY


def add(a, b):
    a, b = _v(a), _v(b)
    v = a.v + b.v
    return V(v, a.e + b.e + _r(v))


def sub(a, b):
    return add(a, -_v(b))


def mul(a, b):
    a, b = _v(a), _v(b)
    v = a.v * b.v
    return V(v, a.e * b.v.detach().abs() + b.e * a.v.detach().abs() + _r(v))


def div(a, b):
    a, b = _v(a), _v(b)
    v = a.v / b.v
    return V(v, (a.e + b.e * v.detach().abs()) / b.v.detach().abs() + _r(v))


def exp(a):
    v = torch.exp(a.v)
    return V(v, a.e * v.detach() + 2 * _r(v))


def log(a):
    v = torch.log(a.v)
    return V(v, a.e / a.v.detach().abs() + 2 * _r(v))


def where(c, a, b):
    a, b = _v(a), _v(b)
    return V(torch.where(c, a.v, b.v), torch.where(c, a.e, b.e))


def vsum(a, dim, L):
    """sum over `dim` through a serial float32 chain of at most L additions"""
    return V(a.v.sum(dim), a.e.sum(dim) + L * U32 * a.v.detach().abs().sum(dim) + TINY)


def image_of(R, row_div, n_img):
    """image of row r: (r / row_div) % n_img   (row_div = 1: sample-major rows n B + b; row_div = N: batch-major b N + n)"""
    return (torch.arange(R) // row_div) % n_img


def sigmoid(g):
    """1 / (1 + expf(-g)) as the kernels evaluate it"""
    return div(1.0, add(1.0, exp(-_v(g))))


# ---- element-wise stages -------------------------------------------------------------------------------------------------------------------
def add_image_rows(H, img, row_div, n_img):
    """H[r] + img[image of r]"""
    return add(H, d(img)[image_of(H.shape[0], row_div, n_img)])


def relu_copy(x):
    """max(x, 0); the sign of a zero result is not defined (fmaxf(-0, +0) may return either)"""
    return torch.clamp_min(d(x), 0.0)


def glu_residual(H, T, gate, row_div, n_img):
    """H + T sigmoid(gate[image of r]), the kernel's form T / (1 + expf(-gate))"""
    g = d(gate)[image_of(H.shape[0], row_div, n_img)]
    return add(H, div(T, add(1.0, exp(V(-g)))))


def glu_bwd(g_h, t3, gate, row_div, n_img):
    """reverse of glu_residual: (g_t3 = g_h s, g_gate_rows = g_h t3 s (1 - s))"""
    s = sigmoid(d(gate)[image_of(g_h.shape[0], row_div, n_img)])
    return mul(g_h, s), mul(mul(mul(g_h, t3), s), sub(1.0, s))


def relu_bwd_add(acc, g, h):
    """acc + g [h > 0]"""
    return add(acc, where(d(h) > 0, g, torch.zeros_like(d(g))))


# ---- the coupling --------------------------------------------------------------------------------------------------------------------------
def pad_cols(n):
    return (n + 63) // 64 * 64


def t_max(dim, first):
    return (dim - first + 1) // 2


def _cols(first, T):
    return first + 2 * torch.arange(T)


def scale_of(us):
    """(sig, scale) of the unconstrained scale: sig = sigmoid(us + 2), scale = sig + 1e-3"""
    sig = sigmoid(add(us, 2.0))
    return sig, add(sig, C1E3)


def pad64(x, ld=None):
    """x [R, dim] zero-padded to [R, ld]"""
    R, dim = x.shape
    out = torch.zeros(R, ld or pad_cols(dim), dtype=_DT[0])
    out[:, :dim] = d(x)
    return out


def _padded(R, ld, cols, base, vals):
    """[R, ld] V: `base` (a [R, dim] tensor, exact) with the columns `cols` replaced by the V `vals`, zero beyond"""
    v = torch.cat([d(base), torch.zeros(R, ld - base.shape[1], dtype=_DT[0])], 1)
    return V(v.index_copy(1, cols, vals.v), torch.zeros(R, ld, dtype=_DT[0]).index_copy(1, cols, vals.e))


def coupling(u, prm, dim, first, T, inverse, seed=None):
    """(y [R, ld], logdet [R]) of mhe_glow_coupling_f32 (u: a tensor, or a V whose transform columns carry an error already): transform feature j is column first + 2 j, prm = [shift (T) | us (T) | ...];
    forward y_t = u_t scale + shift, logdet + sum log scale; inverse y_t = (u_t - shift) / scale, logdet - sum log scale.  The row sum runs
    over ld / 64 values per lane and the six steps of the wave's butterfly"""
    u = _v(u)
    R, ld = u.v.shape[0], pad_cols(dim)
    cols = _cols(first, T)
    shift, us = d(prm)[:, :T], d(prm)[:, T:2 * T]
    _, scale = scale_of(us)
    ut = V(u.v[:, cols], u.e[:, cols])
    yt = div(sub(ut, shift), scale) if inverse else add(mul(ut, scale), shift)
    ls = vsum(log(scale), 1, ld // 64 + 6)
    seed = torch.zeros(R, dtype=_DT[0]) if seed is None else d(seed)
    return _padded(R, ld, cols, u.v[:, :dim], yt), add(seed, -ls if inverse else ls)


def coupling_inv_bwd(v, prm, g_y, dim, first, T, a_q=None, ldp=None):
    """reverse of the inverse coupling: y_t = (v_t - shift) / scale and log q gains + sum log scale; a_q [R] = dL/dlog q per row (a V, or
    None): g_v = g_y / scale on the transform columns (identity columns pass through), g_prm [R, ldp] = [-g_v | (-g_v (v - shift) / scale +
    a_q / scale) sig (1 - sig) | 0]"""
    R, ld, ldp = v.shape[0], pad_cols(dim), ldp or pad_cols(2 * T)
    cols = _cols(first, T)
    shift, us = d(prm)[:, :T], d(prm)[:, T:2 * T]
    sig, scale = scale_of(us)
    gv = div(d(g_y)[:, cols], scale)
    a_q = V(torch.zeros(R, dtype=_DT[0])) if a_q is None else a_q
    a = V(a_q.v[:, None], a_q.e[:, None])
    inner = add(div(mul(-gv, sub(d(v)[:, cols], shift)), scale), div(a, scale))
    g_us = mul(mul(inner, sig), sub(1.0, sig))
    g_prm = V(torch.cat([-gv.v, g_us.v, torch.zeros(R, ldp - 2 * T, dtype=_DT[0])], 1), torch.cat([gv.e, g_us.e, torch.zeros(R, ldp - 2 * T, dtype=_DT[0])], 1))
    return _padded(R, ld, cols, d(g_y)[:, :dim], gv), g_prm


def coupling_fwd_bwd(v, prm, g_y, dim, first, T, a_p=None, ldp=None):
    """reverse of the forward coupling: y_t = v_t scale + shift and log p gains + sum log scale; a_p [R] = dL/dlog p per row or None:
    g_v = g_y scale, g_prm [R, ldp] = [g_y | (g_y v + a_p / scale) sig (1 - sig) | 0]"""
    R, ld, ldp = v.shape[0], pad_cols(dim), ldp or pad_cols(2 * T)
    cols = _cols(first, T)
    us = d(prm)[:, T:2 * T]
    sig, scale = scale_of(us)
    gy = d(g_y)[:, cols]
    a = torch.zeros(R, 1, dtype=_DT[0]) if a_p is None else d(a_p)[:, None]
    g_us = mul(mul(add(mul(gy, d(v)[:, cols]), div(a, scale)), sig), sub(1.0, sig))
    g_prm = V(torch.cat([gy, g_us.v, torch.zeros(R, ldp - 2 * T, dtype=_DT[0])], 1), torch.cat([torch.zeros_like(gy), g_us.e, torch.zeros(R, ldp - 2 * T, dtype=_DT[0])], 1))
    return _padded(R, ld, cols, d(g_y)[:, :dim], mul(gy, scale)), g_prm


def base_density_bwd(zp, g_z, g_logp, dim):
    """g_y [R, ld] = g_z - g_logp[r] z on the padded rows, padding columns zero (g_z [R, dim] or None, g_logp [R] or None)"""
    R, ld = zp.shape
    z = d(zp)[:, :dim]
    gz = torch.zeros_like(z) if g_z is None else d(g_z)
    a = torch.zeros(R, 1, dtype=_DT[0]) if g_logp is None else d(g_logp)[:, None]
    g = sub(gz, mul(a, z))
    return V(torch.cat([g.v, torch.zeros(R, ld - dim, dtype=_DT[0])], 1), torch.cat([g.e, torch.zeros(R, ld - dim, dtype=_DT[0])], 1))


def finish(zp, logdet, dim, sign, parts, host_const=0.0):
    """log_prob[r] = -|z|^2 / 2 - dim / 2 log(2 pi) + sign (logdet[r] + c), c = host_const + sum_i sign parts[i] added one by one; |z|^2 is
    an fma chain of ld / 64 terms per lane and the six steps of the wave's butterfly"""
    z = d(zp)[:, :dim]
    sq = vsum(V(z * z), 1, pad_cols(dim) // 64 + 6)
    c = V(torch.tensor(float(host_const), dtype=_DT[0]))
    for p in d(parts).reshape(-1):
        c = add(c, sign * p)
    base = sub(mul(-0.5, sq), mul(0.5 * dim, LOG2PI))
    return add(base, mul(sign, add(logdet, c)))


# ---- the per-image reverse stages of the one-launch kernel's tape -----------------------------------------------------------------------------
def rows_chain(N, C):
    """L of image_rows_bwd_kernel: 4 rows in flight per trip of a row lane, then the nl lanes folded serially"""
    nl = 512 // (C // 4)
    return 4 * -(-N // (4 * nl)) + nl


def glu_bwd_sum(g_h, t3, gate, N, B):
    """rows r = n B + b: (g_t3 = g_h s [N B, C], gct[b] = s (1 - s) sum_n g_h t3, bsum[b] = s sum_n g_h), s = sigmoid(gate[b])"""
    C = g_h.shape[1]
    s = sigmoid(d(gate))
    gh, t = d(g_h).view(N, B, C), d(t3).view(N, B, C)
    L = rows_chain(N, C)
    gt3 = mul(gh, V(s.v[None], s.e[None]))
    gct = mul(mul(s, sub(1.0, s)), vsum(V(gh * t), 0, L))
    bsum = mul(s, vsum(V(gh), 0, L))
    return V(gt3.v.reshape(N * B, C), gt3.e.reshape(N * B, C)), gct, bsum


def mask_scale_sum(g, t2, scale, N, B):
    """(g' = g scale [t2 > 0] as stored in bf16 [N B, C] - exact: a bf16 times a float32 is exact in float64, then the kernel's two
    roundings - and bsum[b] = sum_n of those STORED values, as the kernel documents)"""
    C = g.shape[1]
    out = torch.where(d(t2) > 0, d(g) * float(np.float32(scale)), torch.zeros((), dtype=_DT[0]))
    st = stored(out, torch.bfloat16)
    return st, vsum(V(st.view(N, B, C)), 0, rows_chain(N, C))


# ---- the dense layer ----------------------------------------------------------------------------------------------------------------------
def linear(x, w, bias=None, relu=False):
    """(act(x w^T + b), sum_k |x w| + |b|)"""
    y, mag = d(x) @ d(w).t(), d(x).abs() @ d(w).abs().t()
    if bias is not None:
        y, mag = y + d(bias), mag + d(bias).abs()
    return (torch.relu(y) if relu else y), mag


def linear_bound(mag, K):
    """per wave a chain of K / 4 fused steps (K / 16 instructions of four products each), three LDS adds, the bias, + 2 slack; the 128 x 128
    fallback walks K in one chain of fused steps of at most four products, so the same count covers it"""
    return (K / 4 + 6) * U32 * mag
