"""The rule of atdn_pose_graph_terms / atdn_pose_graph_solve (include/atdn_hip.h) restated independently of the library:
float64, every operation on its own, every sum in the rule's order — no `@`, `einsum` or `dot`, whose order and fusing are not
the rule's. The edge phase is NumPy, vectorised over the edges (element-wise operations only); the gathers, the block LDL^T,
its sweeps and the conjugate gradient are loops over plain Python floats (IEEE float64, never fused). Seeded scenes, and
`check_case`, which asserts on this helper ALONE before anything is compared with it: every comparison the rule takes (accept or
reject, pivots, the CG stops) has a relative margin >= MIN_MARGIN, at least one step is accepted, and a case that claims a
rejected step, an early CG stop or a CG cap really takes that branch. `check_driver_case` does the same for the two scenes
that accept no step: a factorisation that fails on an exactly zero pivot (`stalled`) and a right-hand side that is exactly zero
(`optimum`). The third such branch of the solver, the curvature stop of the CG (p.Ap <= 0, `info["cg_curvature"]`), is claimed
by NO case: the system is positive semi-definite by construction and no scene was found that takes the stop with a margin."""
import functools

import numpy as np

MIN_MARGIN = 1e-9
DBL_MAX = float(np.finfo(np.float64).max)
EDGE_SIGMA = {"odometry": (1e-3, 1e-2), "loop": (1e-2, 1e-1)}   # rad, m: the scenes' weights are 1 / sigma^2


# ------------------------------------------------------------------ the rule
def _dot3(a0, b0, a1, b1, a2, b2):
    x, y, z = a0 * b0, a1 * b1, a2 * b2
    xy = x + y
    return xy + z


def _atb(A, B):
    return [[_dot3(A[0][a], B[0][b], A[1][a], B[1][b], A[2][a], B[2][b]) for b in range(3)] for a in range(3)]


def tree_sum(values):
    """chunks of 256 (+0.0 beyond the end), the binary tree of strides 1 .. 128, the chunk sums in chunk order"""
    v = np.asarray(values, dtype=np.float64)
    n = len(v)
    chunks = (n + 255) // 256
    w = np.zeros(chunks * 256)
    w[:n] = v
    w = w.reshape(chunks, 256).copy()
    stride = 1
    while stride < 256:
        w[:, ::2 * stride] = w[:, ::2 * stride] + w[:, stride::2 * stride]
        stride *= 2
    total = w[0, 0]
    for c in range(1, chunks):
        total = total + w[c, 0]
    return float(total)


def _split(X):
    """[n,12] internal poses -> (R as 3 x 3 lists of arrays, t as a list of arrays)"""
    return [[X[:, 3 * a + b] for b in range(3)] for a in range(3)], [X[:, 9 + a] for a in range(3)]


def _internal(p32):
    p = np.asarray(p32, dtype=np.float32).reshape(-1, 12).astype(np.float64)
    return np.stack([p[:, 4 * a + b] for a in range(3) for b in range(3)] + [p[:, 4 * a + 3] for a in range(3)], axis=1)


def _public(X):
    return np.stack([X[:, 3 * a + b] if b < 3 else X[:, 9 + a] for a in range(3) for b in range(4)], axis=1).astype(np.float32)


def _residual(Xi, Xj, Z32, wr, wt, robust, q):
    Ri, ti = _split(Xi)
    Rj, tj = _split(Xj)
    Z = np.asarray(Z32, dtype=np.float32).reshape(-1, 12).astype(np.float64)
    Rz = [[Z[:, 4 * a + b] for b in range(3)] for a in range(3)]
    tz = [Z[:, 4 * a + 3] for a in range(3)]
    M = _atb(Ri, Rj)
    Re = _atb(Rz, M)
    d = [tj[a] - ti[a] for a in range(3)]
    tm = [_dot3(Ri[0][a], d[0], Ri[1][a], d[1], Ri[2][a], d[2]) for a in range(3)]
    u = [tm[a] - tz[a] for a in range(3)]
    te = [_dot3(Rz[0][a], u[0], Rz[1][a], u[1], Rz[2][a], u[2]) for a in range(3)]
    av = [0.5 * (Re[2][1] - Re[1][2]), 0.5 * (Re[0][2] - Re[2][0]), 0.5 * (Re[1][0] - Re[0][1])]
    aa = _dot3(av[0], av[0], av[1], av[1], av[2], av[2])
    tt = _dot3(te[0], te[0], te[1], te[1], te[2], te[2])
    ca, ct = wr * aa, wt * tt
    c = ca + ct
    with np.errstate(all="ignore"):
        s = q + c
        f = q / s
        qc = q * c
        omega = np.where(robust, f * f, 1.0)
        cost = np.where(robust, qc / s, c)
    return dict(Rz=Rz, Re=Re, tm=tm, r=av + te, c=c, cost=cost, omega=omega)


def _jtwj(X, w, Y):
    out = [[None] * 6 for _ in range(6)]
    for a in range(6):
        for b in range(6):
            s = None
            for k in range(6):
                wx = w[k] * X[k][a]
                t = wx * Y[k][b]
                s = t if s is None else s + t
            out[a][b] = s
    return out


def _blocks(o, wr, wt):
    Re, Rz, tm = o["Re"], o["Rz"], o["tm"]
    zero = np.zeros_like(wr)
    t01 = Re[0][0] + Re[1][1]
    tr = t01 + Re[2][2]
    Ji = [[zero] * 6 for _ in range(6)]
    Jj = [[zero] * 6 for _ in range(6)]
    G = [[None] * 3 for _ in range(3)]
    for a in range(3):
        for b in range(3):
            dg = tr - Re[a][a]
            G[a][b] = dg if a == b else -Re[a][b]
            Jj[a][b] = 0.5 * dg if a == b else -0.5 * Re[b][a]
            Jj[3 + a][3 + b] = Re[a][b]
    S = [[zero, -tm[2], tm[1]], [tm[2], zero, -tm[0]], [-tm[1], tm[0], zero]]
    Pm = _atb(Rz, S)
    for a in range(3):
        for b in range(3):
            gr = _dot3(G[a][0], Rz[b][0], G[a][1], Rz[b][1], G[a][2], Rz[b][2])
            Ji[a][b] = -0.5 * gr
            Ji[3 + a][b] = Pm[a][b]
            Ji[3 + a][3 + b] = -Rz[b][a]
    owr, owt = o["omega"] * wr, o["omega"] * wt
    w = [owr, owr, owr, owt, owt, owt]
    Aii, Ajj, Aij = _jtwj(Ji, w, Ji), _jtwj(Jj, w, Jj), _jtwj(Ji, w, Jj)
    for a in range(6):                                      # a <= b computed, the rest mirrored
        for b in range(a):
            Aii[a][b] = Aii[b][a]
            Ajj[a][b] = Ajj[b][a]
    g = []
    for J in (Ji, Jj):
        ga = []
        for a in range(6):
            s = None
            for k in range(6):
                wj = w[k] * J[k][a]
                t = wj * o["r"][k]
                s = t if s is None else s + t
            ga.append(s)
        g.append(ga)
    pack = lambda A: np.stack([np.stack(row, axis=1) for row in A], axis=1)   # noqa: E731  [Ea,6,6]
    return pack(Aii), pack(Ajj), pack(Aij), np.stack(g[0], axis=1), np.stack(g[1], axis=1)


def _ldl(A, margins):
    """the 6 x 6 LDL^T of the lower triangle of A (lists of floats) -> (L, d, ok)"""
    L = [[0.0] * 6 for _ in range(6)]
    d = [0.0] * 6
    ok = True
    for j in range(6):
        dj = A[j][j]
        for k in range(j):
            ld = L[j][k] * d[k]
            lld = L[j][k] * ld
            dj = dj - lld
        ok = ok and dj > 0.0
        margins.append(abs(dj) / abs(A[j][j]) if A[j][j] != 0.0 else 0.0)
        d[j] = dj
        for i in range(j + 1, 6):
            l = A[i][j]
            for k in range(j):
                ld = L[j][k] * d[k]
                lld = L[i][k] * ld
                l = l - lld
            L[i][j] = l / dj if dj != 0.0 else float("nan")
    return L, d, ok


def _ldl_solve(L, d, b):
    y = [0.0] * 6
    for i in range(6):
        v = b[i]
        for k in range(i):
            ly = L[i][k] * y[k]
            v = v - ly
        y[i] = v
    y = [y[i] / d[i] for i in range(6)]
    for i in range(5, -1, -1):
        v = y[i]
        for k in range(i + 1, 6):
            ly = L[k][i] * y[k]
            v = v - ly
        y[i] = v
    return y


def _seq(terms):
    s = None
    for t in terms:
        s = t if s is None else s + t
    return s


class _Graph:
    """One graph: the classification of its edges, the incidence lists, the cost, the linearisation, the solver."""

    def __init__(self, poses, index, meas, weight, robust, fixed, scale):
        self.poses32 = np.asarray(poses, dtype=np.float32).reshape(-1, 12)
        self.N = N = len(self.poses32)
        index = np.asarray(index).reshape(2, -1)
        self.E = E = index.shape[1]
        self.meas = np.asarray(meas, dtype=np.float32).reshape(E, 12)
        self.w = np.asarray(weight, dtype=np.float64).reshape(E, 2)
        self.robust = np.zeros(E, bool) if robust is None else np.asarray(robust).reshape(E) != 0
        self.q = float(scale) * float(scale)
        i, j = index[0].astype(np.int64), index[1].astype(np.int64)
        wr, wt = self.w[:, 0], self.w[:, 1]
        with np.errstate(invalid="ignore"):
            ok = ((i >= 0) & (i < N) & (j >= 0) & (j < N) & (i != j) & (wr >= 0) & (wr <= DBL_MAX) & (wt >= 0) & (wt <= DBL_MAX))
        self.valid = ok
        self.ei, self.ej = np.where(ok, i, 0), np.where(ok, j, 0)
        self.active = np.flatnonzero(ok & ((wr > 0) | (wt > 0)))          # ascending edge numbers
        self.inc = [[] for _ in range(N)]                                  # (position among the active edges, side)
        for pos, e in enumerate(self.active):
            self.inc[self.ei[e]].append((pos, 0))
            self.inc[self.ej[e]].append((pos, 1))
        held = np.zeros(N, bool) if fixed is None else np.asarray(fixed).reshape(N) != 0
        self.free = [bool(len(self.inc[n]) > 0 and not held[n]) for n in range(N)]
        self.margins = []

    def _edges(self, X):
        e = self.active
        return _residual(X[self.ei[e]], X[self.ej[e]], self.meas[e], self.w[e, 0], self.w[e, 1], self.robust[e], self.q)

    def cost(self, X, res=None):
        o = self._edges(X) if res is None else res
        shares = [_seq([float(o["cost"][pos]) for pos, side in self.inc[n] if side == 0]) or 0.0 for n in range(self.N)]
        return tree_sum(shares)

    def chi2(self, poses32):
        X = _internal(poses32)
        out = np.zeros(self.E)
        e = np.flatnonzero(self.valid)
        o = _residual(X[self.ei[e]], X[self.ej[e]], self.meas[e], self.w[e, 0], self.w[e, 1], np.zeros(len(e), bool), self.q)
        out[e] = o["c"]
        return out

    def linearise(self, X):
        e = self.active
        o = self._edges(X)
        Aii, Ajj, Aij, gi, gj = _blocks(o, self.w[e, 0], self.w[e, 1])
        N = self.N
        self.D, self.g, self.U = [None] * N, [None] * N, [None] * N
        self.C = Aij.tolist()
        for n in range(N):
            if not self.free[n]:
                continue
            link = n + 1 < N and self.free[n + 1]
            D = g = U = None
            for pos, side in self.inc[n]:
                blk, gr = (Ajj[pos], gj[pos]) if side else (Aii[pos], gi[pos])
                D = blk if D is None else D + blk
                g = gr if g is None else g + gr
                other = self.ei[e[pos]] if side else self.ej[e[pos]]
                if link and other == n + 1:
                    t = Aij[pos].T if side else Aij[pos]
                    U = t if U is None else U + t
            self.D[n], self.g[n] = D.tolist(), g.tolist()
            self.U[n] = (np.zeros((6, 6)) if U is None else U).tolist()

    def factor(self, lam):
        N = self.N
        self.L, self.d, self.W = [None] * N, [None] * N, [None] * N
        for n in range(N):
            if not self.free[n]:
                continue
            A = [row[:] for row in self.D[n]]
            for a in range(6):
                l = lam * A[a][a]
                A[a][a] = A[a][a] + l
            if n > 0 and self.free[n - 1]:
                U, W = self.U[n - 1], self.W[n - 1]
                for a in range(6):
                    for b in range(a + 1):
                        s = _seq([U[c][a] * W[c][b] for c in range(6)])
                        A[a][b] = A[a][b] - s
            L, d, ok = _ldl(A, self.margins)
            if not ok:
                return False
            self.L[n], self.d[n] = L, d
            if n + 1 < N and self.free[n + 1]:
                cols = [_ldl_solve(L, d, [self.U[n][a][b] for a in range(6)]) for b in range(6)]
                self.W[n] = [[cols[b][a] for b in range(6)] for a in range(6)]
        return True

    def precondition(self, r):
        N = self.N
        z = [[0.0] * 6 for _ in range(N)]
        for n in range(N):
            if not self.free[n]:
                continue
            y = r[n][:]
            if n > 0 and self.free[n - 1]:
                W, yp = self.W[n - 1], z[n - 1]
                for a in range(6):
                    s = _seq([W[c][a] * yp[c] for c in range(6)])
                    y[a] = y[a] - s
            z[n] = y
        for n in range(N - 1, -1, -1):
            if not self.free[n]:
                continue
            v = _ldl_solve(self.L[n], self.d[n], z[n])
            if n + 1 < N and self.free[n + 1]:
                W, zn = self.W[n], z[n + 1]
                for a in range(6):
                    s = _seq([W[a][c] * zn[c] for c in range(6)])
                    v[a] = v[a] - s
            z[n] = v
        return z

    def apply(self, p, lam):
        N = self.N
        out = [[0.0] * 6 for _ in range(N)]
        for n in range(N):
            if not self.free[n]:
                continue
            D = self.D[n]
            y = []
            for a in range(6):
                terms = []
                for b in range(6):
                    dv = D[a][b]
                    if a == b:
                        l = lam * dv
                        dv = dv + l
                    terms.append(dv * p[n][b])
                y.append(_seq(terms))
            for pos, side in self.inc[n]:
                e = self.active[pos]
                other = int(self.ei[e] if side else self.ej[e])
                if not self.free[other]:
                    continue
                Cm, po = self.C[pos], p[other]
                for a in range(6):
                    t = _seq([(Cm[b][a] if side else Cm[a][b]) * po[b] for b in range(6)])
                    y[a] = y[a] + t
            out[n] = y
        return out

    def dot(self, a, b):
        return tree_sum([_seq([a[n][k] * b[n][k] for k in range(6)]) for n in range(self.N)])

    def _gap(self, a, b):
        m = max(abs(a), abs(b))
        self.margins.append(abs(a - b) / m if m > 0.0 else 1.0)

    def pcg(self, lam, cg_iters, tol2, info):
        N = self.N
        x = [[0.0] * 6 for _ in range(N)]
        r = [[-v for v in self.g[n]] if self.free[n] else [0.0] * 6 for n in range(N)]
        z = self.precondition(r)
        p = [row[:] for row in z]
        rz = self.dot(r, z)
        thr = tol2 * rz
        its = 0
        if not rz > 0.0:
            assert rz == 0.0 and all(v == 0.0 for row in r for v in row), "r.z <= 0 with a non-zero right-hand side"
            info["zero_rhs"] += 1
            return x, its
        stop = "cap"
        for _ in range(cg_iters):
            Ap = self.apply(p, lam)
            pAp = self.dot(p, Ap)
            scale = sum(abs(p[n][k] * Ap[n][k]) for n in range(N) for k in range(6))
            self.margins.append(abs(pAp) / scale if scale > 0.0 else 0.0)
            if not pAp > 0.0:
                stop = "curvature"
                break
            alpha = rz / pAp
            for n in range(N):
                for k in range(6):
                    ap, aAp = alpha * p[n][k], alpha * Ap[n][k]
                    x[n][k] = x[n][k] + ap
                    r[n][k] = r[n][k] - aAp
            its += 1
            z = self.precondition(r)
            rz_new = self.dot(r, z)
            if rz_new != 0.0:                              # r.z == 0 exactly is a stop of its own, with nothing to compare
                self._gap(rz_new, thr)
            if not rz_new > thr:
                stop = "tolerance"
                break
            beta = rz_new / rz
            for n in range(N):
                for k in range(6):
                    bp = beta * p[n][k]
                    p[n][k] = z[n][k] + bp
            rz = rz_new
        info["cg_" + stop] += 1
        return x, its

    def retract(self, X, x):
        T = X.copy()
        ok = True
        for n in range(self.N):
            if not self.free[n]:
                continue
            dl = x[n]
            ok = ok and all(-DBL_MAX <= v <= DBL_MAX for v in dl)
            A = X[n].tolist()
            h = [0.5 * dl[0], 0.5 * dl[1], 0.5 * dl[2]]
            h00, h11, h22 = h[0] * h[0], h[1] * h[1], h[2] * h[2]
            h01 = h00 + h11
            n2 = h01 + h22
            den = 1.0 + n2
            f = 2.0 / den
            K = [[0.0, -h[2], h[1]], [h[2], 0.0, -h[0]], [-h[1], h[0], 0.0]]
            Em = [[0.0] * 3 for _ in range(3)]
            for i in range(3):
                for j in range(3):
                    hh = h[i] * h[j]
                    m = hh - n2 if i == j else K[i][j] + hh
                    fm = f * m
                    Em[i][j] = 1.0 + fm if i == j else fm
            for a in range(3):
                for b in range(3):
                    T[n, 3 * a + b] = _dot3(A[3 * a], Em[0][b], A[3 * a + 1], Em[1][b], A[3 * a + 2], Em[2][b])
                rt = _dot3(A[3 * a], dl[3], A[3 * a + 1], dl[4], A[3 * a + 2], dl[5])
                T[n, 9 + a] = rt + A[9 + a]
        return T, ok


def terms(poses, index, meas, weight, robust=None, scale=1.0):
    """One graph -> (cost, edge_chi2 [E], counts [2])"""
    G = _Graph(poses, index, meas, weight, robust, None, scale)
    valid = int(G.valid.sum())
    return G.cost(_internal(G.poses32)), G.chi2(G.poses32), np.array([valid, G.E - valid], dtype=np.int32)


def solve(poses, index, meas, weight, robust=None, fixed=None, scale=1.0, iters=10, cg_iters=64, cg_tol=1e-8):
    """One graph -> dict(poses [N,12] float32, cost [2], chi2 [E], counts [4], margin, info)"""
    G = _Graph(poses, index, meas, weight, robust, fixed, scale)
    info = dict(rejected=0, failed=0, zero_rhs=0, cg_cap=0, cg_tolerance=0, cg_curvature=0)
    acc = _internal(G.poses32)
    cost_acc = cost0 = G.cost(acc)
    lam, accepted, cg_total, fresh = 1e-3, 0, 0, False
    tol2 = cg_tol * cg_tol
    for _ in range(iters):
        if not fresh:
            G.linearise(acc)
            fresh = True
        ok = G.factor(lam)
        if ok:
            x, its = G.pcg(lam, cg_iters, tol2, info)
            cg_total += its
            trial, ok = G.retract(acc, x)
        accept = False
        if ok:
            c = G.cost(trial)
            if c != cost_acc:
                G._gap(c, cost_acc)
            accept = c < cost_acc
            if accept:
                acc, cost_acc, fresh = trial, c, False
                accepted += 1
            else:
                info["rejected"] += 1
        else:
            info["failed"] += 1
        if accept:
            l = lam / 3.0
            lam = l if l > 1e-9 else 1e-9
        else:
            l = 4.0 * lam
            lam = l if l < 1e6 else 1e6
    out = G.poses32.copy()
    if accepted > 0:
        free = np.array(G.free)
        out[free] = _public(acc)[free]
    valid = int(G.valid.sum())
    return dict(poses=out, cost=np.array([cost0, cost_acc]), chi2=G.chi2(out),
                counts=np.array([valid, G.E - valid, accepted, cg_total], dtype=np.int32),
                margin=min(G.margins) if G.margins else 1.0, info=info)


# ------------------------------------------------------------------ scenes
def rodrigues(v):
    v = np.asarray(v, dtype=np.float64)
    th = float(np.linalg.norm(v))
    if th == 0.0:
        return np.eye(3)
    k = v / th
    K = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    return np.eye(3) + np.sin(th) * K + (1.0 - np.cos(th)) * (K @ K)


def _T(R, t):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return T


def rows(T):
    """[n,4,4] float64 -> [n,12] float32"""
    return np.ascontiguousarray(np.asarray(T)[..., :3, :].reshape(-1, 12).astype(np.float32))


def ring_truth(N, radius=None):
    """N poses once round a ring (about 1 m between neighbours), the camera turning with it and bobbing a little."""
    radius = N / (2.0 * np.pi) if radius is None else radius
    th = 2.0 * np.pi * np.arange(N) / N
    return np.stack([_T(rodrigues([0.05 * np.sin(2 * a), a, 0.0]), [radius * np.sin(a), 0.2 * np.sin(3 * a), radius * np.cos(a)])
                     for a in th])


def ring_scene(N, loops, seed, noise=(0.0, 0.0), drift=(2e-3, 2e-2), wrong=None, loop_noise=(0.0, 0.0)):
    """A ring of N nodes: the chain edges (k, k+1) and the loop edges `loops` (pairs), with measurements of the truth disturbed
    by `noise` = (rad, m) per odometry edge (random plus the same again as a constant bias) and `loop_noise` per loop edge.
    The start is the truth's node 0 followed by the chain of the odometry measurements disturbed by `drift` per step more (so
    that exact measurements still start drifted). `wrong` = (loop number, translation, rotation vector) falsifies one loop.
    -> dict(poses [N,12], index [2,E], meas [E,12], weight [E,2], robust [E] uint8 (the loops), truth [N,4,4], n_chain)"""
    rs = np.random.RandomState(seed)
    truth = ring_truth(N)
    bias_r, bias_t = rs.normal(size=3) * noise[0], rs.normal(size=3) * noise[1]
    pairs = [(k, k + 1) for k in range(N - 1)] + list(loops)
    meas, start = [], [truth[0]]
    for n, (i, j) in enumerate(pairs):
        Z = np.linalg.inv(truth[i]) @ truth[j]
        chain = n < N - 1
        s = noise if chain else loop_noise
        Z = Z @ _T(rodrigues(rs.normal(size=3) * s[0] + (bias_r if chain else 0.0)),
                   rs.normal(size=3) * s[1] + (bias_t if chain else 0.0))
        if wrong is not None and not chain and n - (N - 1) == wrong[0]:
            Z = Z @ _T(rodrigues(wrong[2]), wrong[1])
        meas.append(Z)
        if chain:
            start.append(start[-1] @ Z @ _T(rodrigues(rs.normal(size=3) * drift[0] + drift[0]), rs.normal(size=3) * drift[1]))
    E = len(pairs)
    so, sl = EDGE_SIGMA["odometry"], EDGE_SIGMA["loop"]
    weight = np.array([[1.0 / so[0] ** 2, 1.0 / so[1] ** 2]] * (N - 1) + [[1.0 / sl[0] ** 2, 1.0 / sl[1] ** 2]] * len(loops))
    robust = np.array([0] * (N - 1) + [1] * len(loops), dtype=np.uint8)
    return dict(poses=rows(np.stack(start)), index=np.ascontiguousarray(np.array(pairs, dtype=np.int32).T), meas=rows(np.stack(meas)),
                weight=weight, robust=robust, truth=truth, n_chain=N - 1, E=E, N=N)


def mean_error(poses12, truth):
    p = np.asarray(poses12, dtype=np.float64).reshape(-1, 3, 4)
    return float(np.mean(np.linalg.norm(p[:, :, 3] - truth[:, :3, 3], axis=1)))


def _graph_args(s, robust=False):
    return (s["poses"], s["index"], s["meas"], s["weight"], s["robust"] if robust else None)


# name -> (scene, solver options, the branches the case claims)
def _pair():
    s = ring_scene(2, [], 1, drift=(2e-2, 2e-1))
    return s, dict(iters=6), ()


def _ring5():
    return ring_scene(5, [(4, 0)], 2), dict(iters=4), ("cg_tolerance",)


def _ring65():
    return ring_scene(65, [(64, 0), (40, 8)], 3), dict(iters=6), ("cg_tolerance",)


def _strided():
    """N = E = 257: one above the workgroup's 256 threads, no multiple of 64; few steps and a low cap keep the helper quick."""
    return ring_scene(257, [(256, 1)], 4, drift=(2e-4, 2e-3)), dict(iters=3, cg_iters=2, cg_tol=1e-13), ("cg_cap",)


def _rejected():
    """a start so far off (0.4 rad, 2 m per step) that a Gauss-Newton step overshoots and is rejected"""
    return ring_scene(9, [(8, 0), (4, 1)], 6, drift=(0.4, 2.0)), dict(iters=4), ("rejected",)


def robust_scene(with_wrong=True):
    """N = 33: odometry noise 0.5 mrad / 5 mm per step plus the same as bias, four true loops, one wrong by (3, -1, 2) m and
    about 0.1 rad; loop sigma 0.01 rad / 0.1 m; robust_scale = 5."""
    loops = [(32, 0), (24, 3), (28, 10), (20, 6)] + ([(16, 1)] if with_wrong else [])
    return ring_scene(33, loops, 5, noise=(5e-4, 5e-3), drift=(0.0, 0.0), loop_noise=(1e-3, 1e-2),
                      wrong=(4, [3.0, -1.0, 2.0], [0.06, -0.06, 0.05]) if with_wrong else None)


ROBUST_SCALE = 5.0


def _robust33():
    return robust_scene(), dict(iters=5, scale=ROBUST_SCALE, robust=True), ()


SINGLE_CASES = {"pair": _pair, "ring5": _ring5, "robust33": _robust33, "ring65": _ring65, "strided": _strided,
                "rejected": _rejected}


def _stalled():
    """`pair` with the rotation weight zero: the free node's block is diag(0, wt Re^T Re), whose first pivot is an exact 0.0
    (products with an exact zero), so the factorisation fails on every step and the input comes back."""
    s = ring_scene(2, [], 1, drift=(2e-2, 2e-1))
    s["weight"][:, 0] = 0.0
    return s, dict(iters=3)


def _optimum():
    """N = 4 at the optimum: rotations I, translations (k, 0, 2k), the four edges of the ring with measurements T_i^-1 T_j —
    small integers, exact in float32 — so every residual and every gradient is exactly zero."""
    N, pairs = 4, [(0, 1), (1, 2), (2, 3), (3, 0)]
    T = np.stack([_T(np.eye(3), [k, 0.0, 2.0 * k]) for k in range(N)])
    meas = np.stack([np.linalg.inv(T[i]) @ T[j] for i, j in pairs])
    s = dict(poses=rows(T), index=np.ascontiguousarray(np.array(pairs, dtype=np.int32).T), meas=rows(meas),
             weight=np.array([[1e6, 1e4]] * len(pairs)), robust=np.zeros(len(pairs), np.uint8), truth=T, E=len(pairs), N=N)
    return s, dict(iters=2)


DRIVER_CASES = {"stalled": _stalled, "optimum": _optimum}


def batch_scene():
    """B = 3 graphs of N = 26 nodes and E = 48 edges in one call, every irregularity the rule names: graph 0 a ring with a
    zero-weight edge, a duplicate edge, a backward edge (i > j) and the three kinds of absent edge (an index -1, an index N,
    i == j); graph 1 a hub of degree 22 at node 3, two held nodes and an isolated node (25); graph 2 a chain with a missing link
    (no edge between 11 and 12) bridged by a long-range edge (11, 13) and (10, 12)."""
    N, E = 26, 48
    truth = ring_truth(N)
    rs = np.random.RandomState(11)
    start = [truth[0]]
    for k in range(N - 1):
        Z = np.linalg.inv(truth[k]) @ truth[k + 1]
        start.append(start[-1] @ Z @ _T(rodrigues(rs.normal(size=3) * 2e-3 + 1e-3), rs.normal(size=3) * 2e-2))
    start = np.stack(start)
    chain = [(k, k + 1) for k in range(N - 1)]
    lists = [
        chain + [(25, 0), (5, 6), (9, 4), (20, 2), (-1, 3), (4, N), (7, 7), (12, 19)],
        [(k, k + 1) for k in range(N - 2)] + [(3, k) for k in range(5, 25)] + [(24, 0)],
        [(k, k + 1) for k in range(N - 1) if k != 11] + [(11, 13), (10, 12), (25, 0), (18, 2)],
    ]
    index = np.zeros((3, 2, E), dtype=np.int32)
    meas = np.zeros((3, E, 12), dtype=np.float32)
    weight = np.zeros((3, E, 2))
    robust = np.zeros((3, E), dtype=np.uint8)
    fixed = np.zeros((3, N), dtype=np.uint8)
    fixed[:, 0] = 1
    fixed[1, 13] = 1
    so, sl = EDGE_SIGMA["odometry"], EDGE_SIGMA["loop"]
    for g, pairs in enumerate(lists):
        pairs = pairs + [(-1, -1)] * (E - len(pairs))               # the lists differ in length: absent edges fill them up
        for e, (i, j) in enumerate(pairs):
            index[g, :, e] = (i, j)
            ok = 0 <= i < N and 0 <= j < N
            Z = np.linalg.inv(truth[i]) @ truth[j] if ok else np.eye(4)
            meas[g, e] = rows(Z[None])[0]
            near = abs(i - j) == 1
            weight[g, e] = (1.0 / so[0] ** 2, 1.0 / so[1] ** 2) if near else (1.0 / sl[0] ** 2, 1.0 / sl[1] ** 2)
            robust[g, e] = 0 if near else 1
    weight[0, 27] = 0.0                                             # graph 0's edge (9, 4): idle
    robust[1] = 0
    poses = np.stack([rows(start)] * 3)
    return dict(poses=poses, index=index, meas=meas, weight=weight, robust=robust, fixed=fixed, truth=truth, N=N, E=E,
                options=dict(iters=3, scale=ROBUST_SCALE))


@functools.lru_cache(maxsize=None)
def check_case(name):
    """The scene `name` and its reference solution, asserted on this helper alone and computed once."""
    scene, opt, claims = SINGLE_CASES[name]()
    opt = dict(opt)
    use_robust = opt.pop("robust", False)
    args = _graph_args(scene, use_robust)
    ref = solve(*args, fixed=_node0(scene["N"]), **opt)
    t = terms(*args, scale=opt.get("scale", 1.0))
    assert ref["margin"] >= MIN_MARGIN, (name, ref["margin"])
    assert ref["counts"][2] >= 1, (name, "no accepted step")
    for claim in claims:
        assert ref["info"][claim] >= 1, (name, claim, ref["info"])
    return dict(scene=scene, args=args, options=opt, solve=ref, terms=t)


@functools.lru_cache(maxsize=None)
def check_driver_case(name):
    """`stalled` and `optimum` with their reference solutions, in the form of `check_case`. Neither accepts a step, and the
    helper reports margin 0.0 for a pivot that is exactly zero, so `stalled` is not held to MIN_MARGIN: what is asserted, on
    this helper alone, is the branch itself — every step fails, or every step has a zero right-hand side and is rejected because
    0 < 0 is false — and that the input poses come back bit for bit."""
    scene, opt = DRIVER_CASES[name]()
    args = _graph_args(scene)
    ref = solve(*args, fixed=_node0(scene["N"]), **opt)
    info, iters, E = ref["info"], opt["iters"], scene["E"]
    assert ref["counts"].tolist() == [E, 0, 0, 0] and np.array_equal(ref["poses"].view(np.uint32), scene["poses"].view(np.uint32))
    assert ref["cost"][0] == ref["cost"][1], (name, ref["cost"])
    if name == "stalled":
        assert info["failed"] == iters and info["rejected"] == 0 and ref["cost"][0] > 0.0, (name, info)
    else:
        assert info["zero_rhs"] == iters and info["rejected"] == iters and info["failed"] == 0, (name, info)
        assert ref["cost"].tolist() == [0.0, 0.0] and ref["margin"] >= MIN_MARGIN, (name, ref["cost"], ref["margin"])
    return dict(scene=scene, args=args, options=opt, solve=ref, terms=terms(*args))


# The float32 round-off of the public poses and measurements: the mean position error (m) that this helper's converged solution
# (8 steps) of a consistent scene leaves — exact measurements of the truth rounded to float32, a drifted start, so the optimum
# is the truth with cost 0. Measured on the helper; the tests allow 4 times as much.
TRUTH_ROUNDOFF = {"ring5": 4.85e-8, "ring65": 4.89e-7}


@functools.lru_cache(maxsize=None)
def truth_case(name):
    scene, _, _ = SINGLE_CASES[name]()
    args = _graph_args(scene)
    return dict(scene=scene, args=args, solve=solve(*args, fixed=_node0(scene["N"]), iters=8))


def _node0(N):
    f = np.zeros(N, dtype=np.uint8)
    f[0] = 1
    return f


@functools.lru_cache(maxsize=None)
def check_batch():
    s = batch_scene()
    opt = s["options"]
    refs = [solve(s["poses"][g], s["index"][g], s["meas"][g], s["weight"][g], s["robust"][g], s["fixed"][g], **opt)
            for g in range(3)]
    for g, r in enumerate(refs):
        assert r["margin"] >= MIN_MARGIN, (g, r["margin"])
        assert r["counts"][2] >= 1, (g, "no accepted step")
    assert refs[0]["counts"][1] == 3 + (s["E"] - 33) and max(len(x) for x in _Graph(
        s["poses"][1], s["index"][1], s["meas"][1], s["weight"][1], None, s["fixed"][1], 1.0).inc) >= 20
    return dict(scene=s, options=opt, solve=refs)


def stack(refs, key):
    return np.stack([r[key] for r in refs])
