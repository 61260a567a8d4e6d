"""Float64 reference of the Procrustes alignment (csrc/procrustes.hip) that is DEFINED on degenerate rows, the bounds of an f32 evaluation
against it, a plain numpy restatement of the kernels' f32 arithmetic, and the cases of tests/test_gpu_aligned_edges.py.  A helper module, not a
test: tests/test_procrustes_ref_host.py checks it on the CPU, tests/test_gpu_aligned_edges.py checks the kernels against it.  The full-rank
reference is align_f64 of tests/test_aligned_oracle.py, unchanged.

Per row, A = target (P x 3), C = hypothesis (P x 3), both f32 and taken as exact:
    t1 = mean A, a = A - t1, s1 = |a|_F + 1e-8, A0 = a / s1;   t2 = mean C, x = C - t2, s2 = |x|_F + 1e-8, B0 = x / s2
    M = A0^T B0 = U S V^T (sigma1 >= sigma2 >= sigma3),  R = U V^T,  s = tr S,  out_p = k R x_p + t1,  k = s s1 / s2

Classes (classify).  `full`: sigma3 >= 1e-3 sigma1.  `rank2`, `rank1`, `rank0`: the trailing singular values are zero EXACTLY in the f32
inputs; evaluated in f64 such a configuration leaves at most P 2^-53 (offset / extent) <= 1024 * 1.1e-16 * 100 ~ 1e-11 of sigma1, so "exact"
is read as <= EXACT = 1e-10 sigma1, and the leading singular values must again be >= 1e-3 sigma1.  Everything in between - a deficiency that
is only as good as f32 noise, a determinant sign that rests on rounding - raises: no test may hold such a row.

What the definition determines (candidates):
    full    one result; R = U V^T is unique also with repeated singular values
    rank2   two: R+- = u1 v1^T + u2 v2^T +- u3 v3^T (u3, v3 the null vectors); out+ = out- when the hypothesis is itself planar (x_p . v3 = 0)
    rank1   s = sigma1, R v1 = u1, and out_p = k (x_p . v1) u1 + t1 when the hypothesis is collinear (then x_p is along v1)
    rank0   s = 0, out = t1

Bounds.  u = 2^-24 (f32 unit roundoff), gamma(n) = n u / (1 - n u), first order in u.  d(P) is the depth of the kernels' f32 sums: rows_kernel
(P <= 32) runs a serial chain of P fmas, d = P; wave_kernel runs ceil(P / 64) fmas per lane and six butterfly steps, d = ceil(P / 64) + 6.
  Centring.  The f32 mean t2^ is a depth-d sum and one division: |t2^ - t2| <= f = (d + 1) u max|C| per coordinate.  x^_p = fl(C_p - t2^) =
    x_p - (t2^ - t2) + r_p, |r_p| <= u |x_p|.  The target's mean is summed in f64 and rounded once: |t1^ - t1| <= e1 = u |t1|; a^, s1^ and
    A0^ = fl(a^ / s1^) carry 3 u relative in all.
  Accumulation.  M^ = sum_p A0^_p x^_p^T by fma chains of depth d: |dM_acc| <= gamma(d) sum_p |A0_p| |x_p|^T.  The CONSTANT parts of the
    centring errors drop out of M to first order (sum_p a_p = 0 = sum_p x_p); what remains is (P e1 / s1 + 2 u sum_p |A0_p|) f^T, and the
    roundings of A0^ and x^: 3 u sum_p |A0_p| |x_p|^T.  In normalised units (divide by s2):
        E = (gamma(d) + 3 u) sum_p |A0_p| |B0_p|^T + (P e1 / s1 + 2 u sum_p |A0_p|) (f / s2)^T        (elementwise),  |dM| <= E
    s1^ and s2^ scale M^ as a whole: no effect on R; they reach s (below) and cancel out of k except through s2^^2 = q^.
  Polar sensitivity.  |dR|_2 <= sqrt2 |dM|_F / (sigma2 + sigma3) to first order (the polar factor of a nonsingular matrix; for rank2 the same
    with sigma3 = 0, to the candidate of the perturbed matrix's determinant sign, both candidates being limits of nonsingular matrices).  The
    kernel's Jacobi sweep stops at off-diagonals below 1e-13 of the diagonal of M^T M: the Gram-Schmidt of M v_i then leaves at most
    1e-13 sigma1^2 (1 / (sigma1 sigma2) + 1 / (sigma1 sigma3) + 1 / (sigma2 sigma3)) (without the sigma3 terms where u3 is completed by the cross
    product).  dR = sqrt2 |E|_F / (sigma2 + sigma3) + that;  R is stored in f32: R_bound = dR + u  (absolute, |R_ij| <= 1).
    rank1: |R^ v1 - u1| <= |u1^ - u1| + |v1^ - v1| <= 2 sqrt2 |dM| / (sigma1 - |dM|) -> 4 |E|_F / sigma1 (Wedin, gap sigma1), + sqrt3 u stored.
    Orthogonality: R^ is orthogonal in f64 and rounded to f32, |R^T R - I|_ij <= sqrt3 u < R_bound; the tests assert R_bound.
  Scale.  d tr S = tr(R^T dM): |d tr S| <= sqrt3 |E|_F.  q^ = sum x^^2 by a depth-d chain, its inputs rounded once (2 u), the constant part of
    the centring error second order but not small far from the origin: rel(q) = gamma(d) + 2 u + 3 P f^2 / q.  s2^ = sqrtf(q^) + 1e-8:
    rel(q) / 2 + 2 u; s1^ = f32(sqrt(f64 sum)) + 1e-8: 3 u.    s_rel = sqrt3 |E|_F / s + 3 u + rel(q) / 2 + 2 u + u (stored)
    k^ = tr S(M^ unnormalised) / q^, computed in f64 and stored once: rel(k) = sqrt3 |E|_F / s + rel(q) + 6 u
  Output.  out^_pi = fma(fl(sum_j R^_ij x^_pj), k^, t1^_i):
        out_bound_pi = k (dR |x_p|_2 + sqrt3 f + 5 u sum_j |R_ij| |x_pj|) + rel(k) |k (R x_p)_i| + u |ref_pi| + u |t1_i|
    the centring term sqrt3 f k is the one that grows when the hypotheses sit far from the origin (|R_i|_1 <= sqrt3); 5 u = the rounding of
    x^ (1), of the stored R (1) and of the three-term sum (3); the final fma adds u |ref|, the rounded t1 u |t1|.
No constant above is fitted to a kernel's output."""
import math

import numpy as np

from test_aligned_oracle import align_f64

U32 = 2.0 ** -24
PSMALL, CH, WAVES, HPW, PMAX = 32, 256, 4, 4, 1024          # the constants of csrc/procrustes.hip
FULL, EXACT = 1e-3, 1e-10
CLASSES = ("rank0", "rank1", "rank2", "full")
SQ2, SQ3 = math.sqrt(2.0), math.sqrt(3.0)


def depth(P):
    return P if P <= PSMALL else -(-P // 64) + 6


def gamma(n):
    return n * U32 / (1.0 - n * U32)


class Solved:
    """the f64 quantities of a batch: target [B,P*3], pred [N,B,P*3] (every field [N,B,...]).  depth_of: the depth d(P) of the f32 sums the
    bounds are evaluated for (default: the kernels')"""

    def __init__(self, target, pred, depth_of=None):
        self.depth_of = depth_of or depth
        target, pred = np.asarray(target), np.asarray(pred)
        self.N, self.B = pred.shape[:2]
        self.P = P = target.reshape(self.B, -1).shape[1] // 3
        A = target.astype(np.float64).reshape(1, self.B, P, 3)
        Cm = pred.astype(np.float64).reshape(self.N, self.B, P, 3)
        self.t1, t2 = A.mean(2, keepdims=True), Cm.mean(2, keepdims=True)
        a, self.x = A - self.t1, Cm - t2
        self.s1 = np.sqrt((a ** 2).sum((2, 3), keepdims=True)) + 1e-8
        self.s2 = np.sqrt((self.x ** 2).sum((2, 3), keepdims=True)) + 1e-8
        self.A0, self.B0 = a / self.s1, self.x / self.s2
        self.M = np.swapaxes(np.broadcast_to(self.A0, self.B0.shape), 2, 3) @ self.B0
        self.U, self.S, self.Vt = np.linalg.svd(self.M)
        self.cmax = np.abs(Cm).max((2, 3))
        self.rank = self._rank()

    def _rank(self):
        s1 = self.S[..., 0]
        safe = np.where(s1 > 0, s1, 1.0)
        rel = self.S / safe[..., None]
        zero = (rel <= EXACT) | (s1 <= 0)[..., None]
        big = rel >= FULL
        if not (zero | big).all():
            n, b = np.argwhere(~(zero | big).all(-1))[0]
            raise ValueError(f"ill-posed row (n={n}, b={b}): singular values / sigma1 = {rel[n, b]} lie between exact zero and {FULL}")
        return big.sum(-1)

    def classes(self):
        return np.array(CLASSES, dtype=object)[self.rank]

    # ---- what the definition determines -------------------------------------------------------------------------------------------------
    def sigma(self):
        return np.where(np.arange(3) < self.rank[..., None], self.S, 0.0)          # exact zeros where the class says so

    def R_candidates(self):
        """[2,N,B,3,3]: R+ = U V^T and R- = U diag(1,1,-1) V^T (equal slots for `full`; meaningful for full and rank2 rows)"""
        Rp = self.U @ self.Vt
        Rm = (self.U * np.array([1.0, 1.0, -1.0])) @ self.Vt
        return np.stack([Rp, np.where((self.rank == 2)[..., None, None], Rm, Rp)])

    def k(self):
        return self.sigma().sum(-1)[..., None, None] * self.s1 / self.s2

    def out_candidates(self):
        """[2,N,B,P*3]: the aligned rows of R+-; rank1 rows: k (x . v1) u1 + t1 (the row of a collinear hypothesis); rank0 rows: t1"""
        k = self.k()
        outs = []
        for R in self.R_candidates():
            o = (self.x @ np.swapaxes(R, 2, 3)) * k + self.t1
            u1, v1 = self.U[..., :, 0], self.Vt[..., 0, :]
            o1 = ((self.x * v1[:, :, None, :]).sum(-1, keepdims=True) * u1[:, :, None, :]) * k + self.t1
            o = np.where((self.rank == 1)[..., None, None], o1, o)
            o = np.where((self.rank == 0)[..., None, None], np.broadcast_to(self.t1, o.shape), o)
            outs.append(o.reshape(self.N, self.B, -1))
        return np.stack(outs)

    def hypothesis_rank(self):
        """[N,B]: the rank of the centred hypothesis (same reading of "exact")"""
        sv = np.linalg.svd(self.B0, compute_uv=False)
        return (sv > EXACT * np.maximum(sv[..., :1], 1e-300)).sum(-1) * (sv[..., 0] > 0)

    # ---- bounds (module docstring) -------------------------------------------------------------------------------------------------------
    def _centring(self):
        """f [N,B]: |t2^ - t2| per coordinate;  e1 [1,B,3]: |t1^ - t1|"""
        f = (self.depth_of(self.P) + 1) * U32 * self.cmax
        return f, U32 * np.abs(self.t1[:, :, 0, :])

    def _accumulation(self, f, e1):
        """|E|_F [N,B] of the elementwise bound E on dM (normalised units)"""
        d = self.depth_of(self.P)
        absA, absB = np.abs(np.broadcast_to(self.A0, self.B0.shape)), np.abs(self.B0)
        G = np.swapaxes(absA, 2, 3) @ absB                                                     # sum_p |A0_pi| |B0_pj|
        lead = self.P * e1 / self.s1[:, :, 0, :] + 2 * U32 * np.abs(self.A0).sum(2)            # [1,B,3]
        E = (gamma(d) + 3 * U32) * G + lead[..., :, None] * (f / self.s2[:, :, 0, 0])[..., None, None]
        return np.sqrt((E ** 2).sum((-1, -2)))

    def _polar(self, EF):
        """dR [N,B]: on |dR|_2 (full, rank2), on |R^ v1 - u1| (rank1), 0 (rank0)"""
        sg = self.sigma()
        g1, g2, g3 = sg[..., 0], sg[..., 1], sg[..., 2]
        with np.errstate(divide="ignore", invalid="ignore"):
            jac = 1e-13 * g1 * g1 * (1 / (g1 * g2) + np.where(g3 > 0, 1 / (g1 * g3) + 1 / (g2 * g3), 0.0))
            dR = np.where(self.rank >= 2, SQ2 * EF / (g2 + g3) + jac, 4 * EF / g1)
        return np.where(self.rank == 0, 0.0, dR)

    def _scale(self, EF, f):
        """(rel(k), s_rel, s) [N,B]"""
        d = self.depth_of(self.P)
        q = (self.x ** 2).sum((2, 3))
        ssum = self.sigma().sum(-1)
        with np.errstate(divide="ignore", invalid="ignore"):
            relq = gamma(d) + 2 * U32 + np.where(q > 0, 3 * self.P * f * f / q, 0.0)
            rels = np.where(ssum > 0, SQ3 * EF / ssum, 0.0)
        return rels + relq + 6 * U32, rels + 3 * U32 + relq / 2 + 2 * U32 + U32, ssum

    def _output(self, dR, f, relk):
        """out_bound [N,B,P,3]"""
        k = self.k()[:, :, 0, 0][..., None, None]
        xn = np.sqrt((self.x ** 2).sum(-1))                                                    # [N,B,P]
        absR = np.where((self.rank >= 2)[..., None, None], np.abs(self.R_candidates()).max(0), 1.0)
        Rx = np.abs(self.x) @ np.swapaxes(absR, 2, 3)                                          # sum_j |R_ij| |x_pj|
        oc = self.out_candidates().reshape(2, self.N, self.B, self.P, 3)
        dev, ref = np.abs(oc - self.t1).max(0), np.abs(oc).max(0)                              # |k (R x_p)_i|, |ref_pi|
        ob = k * (dR[..., None, None] * xn[..., None] + SQ3 * f[..., None, None] + 5 * U32 * Rx) + relk[..., None, None] * dev \
            + U32 * ref + U32 * np.abs(self.t1)
        return np.where((self.rank == 0)[..., None, None], U32 * np.abs(np.broadcast_to(self.t1, ob.shape)), ob)

    def bounds(self):
        """dict: 'out' [N,B,P*3], 'R' [N,B] (absolute; rank1: on R v1), 's' [N,B] (absolute = s_rel * s); term by term as in the docstring"""
        f, e1 = self._centring()
        EF = self._accumulation(f, e1)
        dR = self._polar(EF)
        relk, s_rel, ssum = self._scale(EF, f)
        ob = self._output(dR, f, relk)
        Rb = np.where(self.rank >= 2, dR + U32, dR + SQ3 * U32)
        return {"out": ob.reshape(self.N, self.B, -1), "R": Rb, "s": s_rel * ssum}


# ---- the row-level surface ------------------------------------------------------------------------------------------------------------------
def _row(target_row, pred_row):
    return Solved(np.asarray(target_row).reshape(1, -1), np.asarray(pred_row).reshape(1, 1, -1))


def classify(target_row, pred_row):
    """'full', 'rank2', 'rank1' or 'rank0'; raises ValueError on a row that is neither well-posed nor exactly deficient"""
    return str(_row(target_row, pred_row).classes()[0, 0])


def candidates(target_row, pred_row):
    """the results the definition allows: a list of dicts.  full: one {'out','R','s'}; rank2: two; rank1: one {'s','u1','v1','out'} with
    out = None unless the hypothesis is collinear; rank0: one {'s': 0, 'out': t1 repeated}"""
    S = _row(target_row, pred_row)
    cls, s = S.classes()[0, 0], float(S.sigma().sum())
    oc, Rc = S.out_candidates()[:, 0, 0], S.R_candidates()[:, 0, 0]
    if cls == "full":
        return [{"out": oc[0], "R": Rc[0], "s": s}]
    if cls == "rank2":
        return [{"out": oc[i], "R": Rc[i], "s": s} for i in range(2)]
    if cls == "rank1":
        return [{"s": s, "u1": S.U[0, 0, :, 0], "v1": S.Vt[0, 0, 0, :], "out": oc[0] if S.hypothesis_rank()[0, 0] <= 1 else None}]
    return [{"s": 0.0, "out": oc[0]}]


def out_bound(target_row, pred_row):
    """per-element bound on |out - ref| of the row (derived for `full` rows; the deficient classes use the same terms, module docstring)"""
    return _row(target_row, pred_row).bounds()["out"][0, 0]


def R_bound(target_row, pred_row):
    return float(_row(target_row, pred_row).bounds()["R"][0, 0])


def s_bound(target_row, pred_row):
    return float(_row(target_row, pred_row).bounds()["s"][0, 0])


# ---- a plain numpy restatement of the kernels' f32 arithmetic -----------------------------------------------------------------------------------
F32 = np.float32


def _fma(a, b, c):
    """f32 fma: the product of two f32 is exact in f64"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F32)


def _lane_sum(terms, P, fused=None):
    """the kernels' summation order over the points: terms(p) -> f32 [rows]; serial for P <= PSMALL, else 64 lane chains and an xor butterfly.
    fused: (a(p), b(p)) accumulates fma(a, b, acc) instead of acc + terms(p)"""
    def step(acc, p):
        if fused is not None:
            a, b = fused(p)
            return _fma(a, b, acc)
        return (acc + terms(p)).astype(F32)
    probe = np.broadcast_arrays(*fused(0))[0] if fused is not None else terms(0)
    if P <= PSMALL:
        acc = np.zeros_like(probe, dtype=F32)
        for p in range(P):
            acc = step(acc, p)
        return acc
    lanes = []
    for lane in range(64):
        acc = np.zeros_like(probe, dtype=F32)
        for p in range(lane, P, 64):
            acc = step(acc, p)
        lanes.append(acc)
    v = np.stack(lanes, -1)
    for o in (32, 16, 8, 4, 2, 1):
        v = (v + v[..., np.arange(64) ^ o]).astype(F32)
    return v[..., 0]


def polar3(m):
    """csrc/procrustes.hip polar3 in numpy f64, statement by statement: m [3,3] -> R [3,3], s"""
    m = np.asarray(m, np.float64)
    a, v = m.T @ m, np.eye(3)
    for _ in range(8):
        off = a[0, 1] ** 2 + a[0, 2] ** 2 + a[1, 2] ** 2
        dia = a[0, 0] ** 2 + a[1, 1] ** 2 + a[2, 2] ** 2
        if not off > 1e-26 * dia:
            break
        for p, q in ((0, 1), (0, 2), (1, 2)):
            o = 3 - p - q
            apq = a[p, q]
            if apq == 0.0:
                continue
            th = (a[q, q] - a[p, p]) / (2.0 * apq)
            t = 0.5 / th if abs(th) > 1e150 else math.copysign(1.0, th) / (abs(th) + math.sqrt(th * th + 1.0))
            c = 1.0 / math.sqrt(t * t + 1.0)
            sn = t * c
            a[p, p] -= t * apq
            a[q, q] += t * apq
            a[p, q] = a[q, p] = 0.0
            aop, aoq = a[o, p], a[o, q]
            a[o, p] = a[p, o] = c * aop - sn * aoq
            a[o, q] = a[q, o] = sn * aop + c * aoq
            vp, vq = v[:, p].copy(), v[:, q].copy()
            v[:, p], v[:, q] = c * vp - sn * vq, sn * vp + c * vq
    lam, ord_ = [a[0, 0], a[1, 1], a[2, 2]], [0, 1, 2]
    for i, j in ((0, 1), (1, 2), (0, 1)):
        if lam[ord_[i]] < lam[ord_[j]]:
            ord_[i], ord_[j] = ord_[j], ord_[i]
    vc = np.stack([v[:, ord_[i]] for i in range(3)])
    u = np.stack([m @ vc[i] for i in range(3)])
    n1 = math.sqrt(float(u[0] @ u[0]))
    tiny = 1e-13 * n1
    u[0] = u[0] / n1 if n1 > 0.0 else np.array([1.0, 0.0, 0.0])
    u[1] -= (u[1] @ u[0]) * u[0]
    n2 = math.sqrt(float(u[1] @ u[1]))
    if n2 > tiny and n2 > 0.0:
        u[1] /= n2
    else:
        ax = np.abs(u[0])
        e = np.zeros(3)
        e[0 if (ax[0] <= ax[1] and ax[0] <= ax[2]) else (1 if ax[1] <= ax[2] else 2)] = 1.0
        u[1] = e - (e @ u[0]) * u[0]
        u[1] /= math.sqrt(float(u[1] @ u[1]))
    u[2] -= (u[2] @ u[0]) * u[0] + (u[2] @ u[1]) * u[1]
    n3 = math.sqrt(float(u[2] @ u[2]))
    u[2] = u[2] / n3 if (n3 > tiny and n3 > 0.0) else np.cross(u[0], u[1])
    r = u.T @ vc
    return r, float((r * m).sum())


def kernel_f32(target, pred):
    """target [B,P*3], pred [N,B,P*3] f32 -> out [N,B,P*3], R [N,B,3,3], s [N,B] (f32): the arithmetic of target_kernel, rows_kernel (P <= 32)
    or wave_kernel and solve(), in their order of operations, the polar factor by polar3 above"""
    target, pred = np.asarray(target, F32), np.asarray(pred, F32)
    N, B = pred.shape[:2]
    A = target.reshape(B, -1, 3)
    P = A.shape[1]
    C = pred.reshape(N, B, P, 3)
    t1 = A.astype(np.float64).mean(1).astype(F32)                                          # [B,3]
    a = (A - t1[:, None]).astype(F32)
    s1 = (np.sqrt((a.astype(np.float64) ** 2).sum((1, 2))).astype(F32) + F32(1e-8)).astype(F32)
    A0 = (a / s1[:, None, None]).astype(F32)
    t2 = (_lane_sum(lambda p: C[:, :, p], P) / F32(P)).astype(F32)                         # [N,B,3]
    x = (C - t2[:, :, None]).astype(F32)
    xs = x.reshape(N, B, P * 3)
    q = np.zeros((N, B), F32)
    if P <= PSMALL:
        for i in range(P * 3):
            q = _fma(xs[..., i], xs[..., i], q)
    else:
        lanes = []                                                                             # three fmas per point, in coordinate order
        for lane in range(64):
            acc = np.zeros((N, B), F32)
            for p in range(lane, P, 64):
                for i in range(3):
                    acc = _fma(x[:, :, p, i], x[:, :, p, i], acc)
            lanes.append(acc)
        v = np.stack(lanes, -1)
        for o in (32, 16, 8, 4, 2, 1):
            v = (v + v[..., np.arange(64) ^ o]).astype(F32)
        q = v[..., 0]
    Ab = np.broadcast_to(A0[None], (N, B, P, 3))
    mr = _lane_sum(None, P, fused=lambda p: (Ab[:, :, p, :, None], x[:, :, p, None, :]))  # [N,B,3,3]
    s2 = (np.sqrt(q).astype(F32) + F32(1e-8)).astype(F32)
    m = mr.astype(np.float64) / s2.astype(np.float64)[..., None, None]
    R64, s64 = np.empty((N, B, 3, 3)), np.empty((N, B))
    for n in range(N):
        for b in range(B):
            R64[n, b], s64[n, b] = polar3(m[n, b])
    R = R64.astype(F32)
    k = (s64 * s1.astype(np.float64)[None] / s2.astype(np.float64)).astype(F32)
    y = ((R[:, :, None, :, 0] * x[..., 0:1]).astype(F32) + (R[:, :, None, :, 1] * x[..., 1:2]).astype(F32)).astype(F32)
    y = (y + (R[:, :, None, :, 2] * x[..., 2:3]).astype(F32)).astype(F32)
    out = _fma(y, np.broadcast_to(k[..., None, None], y.shape), np.broadcast_to(t1[None, :, None, :], y.shape))
    return out.reshape(N, B, P * 3), R, s64.astype(F32)


# ---- the cases of tests/test_gpu_aligned_edges.py ---------------------------------------------------------------------------------------------------
def rot(rng):
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    return q if np.linalg.det(q) > 0 else -q


def hands(rng, B, P, N, far=0.0):
    """_hands of tests/test_gpu_aligned.py (targets ~0.6 m from the origin at a ~0.1 m extent, hypotheses rotated, scaled by 30, shifted and
    perturbed copies); far: the hypotheses additionally sit `far` extents (of ~3 units) from the origin"""
    shape = rng.normal(0, 0.03, (B, P, 3))
    tgt = shape + np.array([0.05, -0.1, 0.6]) + rng.normal(0, 0.02, (B, 1, 3))
    pred = np.empty((N, B, P, 3))
    for b in range(B):
        Q = rot(rng)
        pred[:, b] = (shape[b] @ Q.T) * 30.0 + rng.normal(0, 0.3, (N, 1, 3)) + rng.normal(0, 0.2, (N, P, 3))
    pred += far * 3.0 * np.array([0.6, -0.5, 0.62])
    return tgt.reshape(B, -1).astype(F32), pred.reshape(N, B, -1).astype(F32)


# (N, P) -> the path the pair selects.  rows_kernel: P <= 32, one thread per hypothesis, chunks of CH = 256; wave_kernel: one wave per
# hypothesis, 16 per workgroup (4 waves x 4), `vec` = float2 loads and stores (P*3 even and aligned pointers).
SWEEP = {
    (1, 1): "rows; one chunk, cn = 1; P = 1: rank0 (M = 0, out = t1)",
    (5, 2): "rows; P = 2: rank1 in the inputs, rank 2 at noise level after the f32 centring (u2 from a noise-sized remainder)",
    (3, 3): "rows; P = 3: rank2 in the inputs, full rank at noise level after the f32 centring (u3 from a noise-sized remainder)",
    (4, 4): "rows; the smallest P of full rank",
    (16, 4): "rows; one ragged chunk",
    (17, 21): "rows; the joints' P, odd row stride 63",
    (255, 21): "rows; ragged chunk one short of CH",
    (256, 21): "rows; cn == CH exactly, one workgroup",
    (257, 21): "rows; chunk 1 (blockIdx.x = 1, n0 = 256), ragged cn = 1",
    (513, 21): "rows; chunks 0, 1 full and chunk 2 ragged",
    (3, 31): "rows; P = PSMALL - 1",
    (257, 31): "rows; chunk 1 at an odd row stride 93",
    (1, 32): "rows; P = PSMALL, cn = 1",
    (256, 32): "rows; P = PSMALL and cn == CH: the whole 98 704-byte LDS request is written",
    (257, 32): "rows; P = PSMALL, chunk 1",
    (513, 32): "rows; P = PSMALL, three chunks",
    (1, 33): "wave; the smallest wave row (31 lanes without a point), P*3 odd: vec false; break at h = 1 of wave 0",
    (3, 33): "wave; break at h = 3 inside the first wave",
    (17, 33): "wave; N = 16 k + 1: workgroup 1 holds one row; vec false",
    (5, 49): "wave; vec false; wave 1 breaks at h = 1",
    (16, 63): "wave; vec false, one point short of a full wave; 16 rows = one full workgroup, no break",
    (1, 64): "wave; vec true, one point per lane",
    (17, 64): "wave; vec true, second workgroup",
    (5, 65): "wave; vec false, lane 0 takes a second point",
    (33, 65): "wave; vec false, three workgroups",
    (3, 777): "wave; vec false, 13 points in lanes 0..8, 12 in the others",
    (17, 777): "wave; vec false, second workgroup",
    (5, 778): "wave; vec true (the mesh)",
    (16, 778): "wave; vec true, one full workgroup",
    (1, 1023): "wave; vec false, P = PMAX - 1",
    (3, 1023): "wave; vec false, all four hypotheses slots of wave 0 but one",
    (1, 1024): "wave; vec true, P = PMAX: LDS slices at their sized maximum",
    (33, 1024): "wave; vec true, P = PMAX, three workgroups",
}
FAR = {(257, 21): "rows, chunk 1", (17, 32): "rows, P = PSMALL", (5, 65): "wave, vec false", (3, 778): "wave, vec true",
       (1, 1024): "wave, P = PMAX"}
FAR_EXTENTS = 100.0


def _well_posed(make, seed):
    """the first draw of make(rng) over the seeds seed, seed + 1, ... whose rows classify() all accepts as `full`.  With few points a random
    row is ill-posed now and then (P = 4 leaves three centred points' worth of freedom); such a draw is not a test case"""
    for i in range(64):
        t, h = make(np.random.default_rng(seed + i))
        try:
            if (Solved(t, h).rank == 3).all():
                return t, h
        except ValueError:
            pass
    raise RuntimeError("no well-posed draw")


def sweep_case(N, P, far=False):
    """(target [B,P*3], pred [N,B,P*3]) of a sweep pair; B = 2.  P <= 3 is deficient by construction, P >= 4 is drawn well-posed"""
    seed, ext = 1000 * P + N + (500000 if far else 0), FAR_EXTENTS if far else 0.0
    if P <= 3:
        return hands(np.random.default_rng(seed), 2, P, N, ext)
    return _well_posed(lambda rng: hands(rng, 2, P, N, ext), 100 * seed)


def _grid(rng, shape, lo=-40, hi=40, step=1.0 / 64):
    """f32 values on a dyadic grid (|value| < 1): sums of up to 1024 of them are exact in f32 in any order"""
    return (rng.integers(lo, hi + 1, shape) * step).astype(np.float64)


def _zero_mean(g, step=1.0 / 64):
    """the last point chosen so that every coordinate sums to zero exactly over the points (axis -2)"""
    g = g.copy()
    g[..., -1, :] = -g[..., :-1, :].sum(-2)
    return g


def _cube():
    return np.array([[x, y, z] for x in (-1.0, 1.0) for y in (-1.0, 1.0) for z in (-1.0, 1.0)])


def degenerate_cases():
    """name -> (target [B,P*3] f32, pred [N,B,P*3] f32, class, kind).  kind: 'ambiguous' (rank2, the two candidates' rows differ), 'planar_hyp'
    (rank2, they coincide), 'rank1', 'rank1_collinear_hyp', 'unique' (full).  The planar_* and collinear_* cases are built on dyadic grids
    with zero-sum deviations, so that the kernels' own f32 centring is exact and the deficiency survives it
    (tests/test_procrustes_ref_host.py confirms that with kernel_f32); three_points*, two_points are not (see below)."""
    rng = np.random.default_rng(77)
    cases = {}
    N, B = 5, 2
    off_t, off_h = np.array([0.0625, -0.125, 0.625]), np.array([1.5, -2.25, 0.75])

    def shape(P, flat=None):
        g = _grid(rng, (B, P, 3), -32, 32)
        if flat is not None:
            g[..., flat] = 0.0
        return _zero_mean(g)

    def copies(sh, flat=None):
        """rotated, scaled, perturbed copies of the shape, rounded to the grid, their deviations from off_h summing to zero exactly"""
        h = np.empty((N,) + sh.shape)
        for b in range(B):
            h[:, b] = np.round(((sh[b] @ rot(rng).T) * 8.0 + rng.normal(0, 0.4, (N,) + sh.shape[1:])) * 64.0) / 64.0
        if flat is not None:
            h[..., flat] = 0.0
        return _zero_mean(h) + off_h

    def general(P):
        return _zero_mean(_grid(rng, (N, B, P, 3))) * 8.0 + off_h

    for P in (21, 40):                                                                          # rows_kernel and wave_kernel
        sh = shape(P, flat=2)                                                                   # the target in the plane z = 0.625
        cases[f"planar_target_P{P}"] = (sh * 0.0625 + off_t, copies(sh), "rank2", "ambiguous")
        sh3 = shape(P)
        cases[f"planar_hypothesis_P{P}"] = (sh3 * 0.0625 + off_t, copies(sh3, flat=1), "rank2", "planar_hyp")      # in the plane y = -2.25
        cases[f"planar_both_P{P}"] = (sh * 0.0625 + off_t, copies(sh, flat=1), "rank2", "planar_hyp")
    # P = 3 and P = 2 are hand-like rows, NOT on the grid: deficient exactly in the f32 inputs, but after the kernels' f32 centring and fma
    # chains M is of full rank at noise level (sigma / sigma1 ~ 1e-8), so polar3 normalises a noise-sized remainder instead of taking its
    # completion branches (those are what planar_target_* - a row of M exactly zero - and collinear_target_* reach).  The comparison stays
    # sound: the hypothesis is planar (collinear), so both rank2 candidates coincide (the rank1 row is determined)
    t3, h3 = hands(rng, 3, 3, 4)
    cases["three_points"] = (t3, h3, "rank2", "planar_hyp")
    t3f, h3f = hands(rng, 2, 3, 4, far=FAR_EXTENTS)
    cases["three_points_far"] = (t3f, h3f, "rank2", "planar_hyp")
    for P in (21, 40):
        line = _zero_mean(_grid(rng, (B, P, 1), -20, 20, 1.0))                                  # integer positions along the line
        t = line * np.array([0.03125, -0.015625, 0.0625]) + off_t
        cases[f"collinear_target_P{P}"] = (t, general(P), "rank1", "rank1")
        hl = _zero_mean(_grid(rng, (N, B, P, 1), -20, 20, 1.0)) * np.array([0.5, 1.0, -0.25]) + off_h
        cases[f"collinear_hypothesis_P{P}"] = (shape(P) * 0.0625 + off_t, hl, "rank1", "rank1_collinear_hyp")
    t2, h2 = hands(rng, 3, 2, 4)
    cases["two_points"] = (t2, h2, "rank1", "rank1_collinear_hyp")
    # repeated singular values: M proportional to an orthogonal matrix
    cube = _cube()
    quarter = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])                    # exact in f32: K = M^T M is a multiple of I
    mirror = np.diag([1.0, -1.0, 1.0])
    for name, flip in (("cube", np.eye(3)), ("cube_mirror", mirror)):
        t = np.stack([cube * 0.0625 + np.array([0.0625, -0.125, 0.625])] * B)
        h = np.empty((N, B, 8, 3))
        for n in range(N):
            for b in range(B):
                Q = quarter if n == 0 else rot(rng)
                h[n, b] = (cube @ flip @ Q.T) * (2.0 if n == 0 else rng.uniform(10, 40)) + (off_h if n == 0 else rng.normal(0, 1, 3))
        cases[name] = (t, h, "full", "unique")
    # nearly planar, well-posed: a flat open hand.  M's smallest singular value goes with the PRODUCT of the two thicknesses, so each
    # point set is 0.06 of its extent thick: sigma3 / sigma1 of a few 1e-3 (classify keeps anything thinner out)
    def flat_hand(P):
        def make(r):
            sh = r.normal(0, 0.03, (B, P, 3)) * np.array([1.0, 1.0, 0.06])
            t = sh @ rot(r).T + np.array([0.05, -0.1, 0.6])
            h = np.empty((N, B, P, 3))
            for b in range(B):
                h[:, b] = (sh[b] @ rot(r).T) * 30.0 + r.normal(0, 0.3, (N, 1, 3)) + r.normal(0, 0.002, (N, P, 3))
            return t.astype(F32).reshape(B, -1), h.astype(F32).reshape(N, B, -1)
        return make
    for P in (21, 778):
        t, h = _well_posed(flat_hand(P), 7700 + P)
        cases[f"nearly_planar_P{P}"] = (t, h, "full", "unique")
    for k, (t, h, c, kind) in cases.items():
        t32, h32 = np.ascontiguousarray(t, F32), np.ascontiguousarray(h, F32)
        if k.startswith(("planar_", "collinear_")):
            assert np.array_equal(t32, t) and np.array_equal(h32, h), k                         # the grid values are f32 numbers
        cases[k] = (t32.reshape(t.shape[0], -1), h32.reshape(h.shape[0], h.shape[1], -1), c, kind)
    return cases


def select(got, cands, bound):
    """per row the candidate closest to `got` in units of the bound: got [N,B,F], cands [2,N,B,F] -> [N,B,F].  A row is compared with the
    candidate that minimises its largest |diff| / bound, so asserting the selected comparison asserts min over the candidates for every row"""
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(np.abs(got[None] - cands) == 0, 0.0, np.abs(got[None] - cands) / bound[None])
    pick = ratio.reshape(*ratio.shape[:3], -1).max(-1).argmin(0)                                # [N,B]
    return np.take_along_axis(cands, pick[None, ..., None], 0)[0], pick
