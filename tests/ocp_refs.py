"""Problems, LDS packing and references for the device tests of csrc/ocp_wave.h's Riccati engine
(tests/test_gpu_ocp_riccati.py) and their host-only checks (tests/test_wave_refs.py).

The problem the header documents, per subsystem:
    minimise  sum_{k<N} 1/2 z_k^T H_k z_k + 1/2 [x_N; 1]^T Pt_N [x_N; 1],   z = [x; u; 1],
    subject to  [x_{k+1}; 1] = M_k z_k,  x_0 = dx0,    M = [[A B c]; [0 0 1]].
Two references that share no code with the kernels: the whole problem as one dense KKT system, solved in float64 and
refined with longdouble residuals; and the textbook Riccati recursion in plain float64 with dense matrices, whose
distance from the first (e_ref) sets the tolerance of the device test."""
import functools

import numpy as np

LD = np.longdouble
ONE_WAVE_N = (1, 2, 3, 4, 21, 22, 30, 31)
TWO_WAVE_N = (32, 33, 62, 63)
TWO_WAVE_SMALL_N = (1, 2, 3, 31)
INSTANCES = 3
FORMS = {"aug": dict(nxa=6, nu=2, halves=1), "s": dict(nxa=5, nu=1, halves=2)}


# ---------------------------------------------------------------------------------------------------------
# the header's layout, restated: packed symmetric index, NodeArr stride, struct field sizes
# ---------------------------------------------------------------------------------------------------------
def tri(n):
    return n * (n + 1) // 2


def hp(i, j):
    return tri(i) + j if i >= j else tri(j) + i


def even(n):
    return (n + 1) & ~1


def node_stride(w):
    """Doubles between the blocks of consecutive nodes of a NodeArr whose element holds w doubles."""
    w2 = (w + 1) & ~1
    return w2 if (w2 // 2) % 2 else w2 + 2


def layout(form, waves):
    nxa, nu = FORMS[form]["nxa"], FORMS[form]["nu"]
    NP, ND = nxa + 1, nxa + nu + 1
    NC, NT = even(NP), tri(ND)
    nmaxs = 32 * waves
    slots = nmaxs * FORMS[form]["halves"]
    swm, swg = node_stride(ND * NC), node_stride(even(NT))
    return dict(nxa=nxa, nu=nu, NP=NP, ND=ND, NC=NC, NT=NT, nmaxs=nmaxs, slots=slots, swm=swm, swg=swg,
                msize=slots * swm, gsize=slots * swg)


# ---------------------------------------------------------------------------------------------------------
# seeded problems
# ---------------------------------------------------------------------------------------------------------
def _spd(rng, n):
    W = rng.standard_normal((n, n)) / np.sqrt(n)
    return W @ W.T + np.eye(n)


def _subsystem(rng, form, N):
    nxa, nu = FORMS[form]["nxa"], FORMS[form]["nu"]
    ny = nxa + nu
    A, B, c = np.zeros((N, nxa, nxa)), np.zeros((N, nxa, nu)), np.zeros((N, nxa))
    for k in range(N):
        n = nxa - 2 if form == "aug" else nxa       # aug: x~ = [x (4); u_prev (2)], the u_prev columns of M are zero
        a = rng.standard_normal((n, n))
        a *= 0.95 * rng.uniform(0.5, 1.0) / np.max(np.abs(np.linalg.eigvals(a)))
        A[k, :n, :n] = a
        B[k, :n] = rng.standard_normal((n, nu))
        c[k, :n] = rng.standard_normal(n)
        if form == "aug":
            B[k, n:] = np.eye(2)                    # the u_prev rows select u_k
    return dict(N=N, nxa=nxa, nu=nu, A=A, B=B, c=c, Hyy=np.array([_spd(rng, ny) for _ in range(N)]),
                g=rng.standard_normal((N, ny)), h0=rng.standard_normal(N), PN=_spd(rng, nxa),
                pN=rng.standard_normal(nxa), cN=rng.standard_normal(), dx0=rng.standard_normal(nxa))


@functools.lru_cache(maxsize=None)
def problem(form, N, inst):
    """The subsystems of instance ``inst`` of a shape (one for "aug", two independent ones for "s")."""
    rng = np.random.default_rng([{"aug": 1, "s": 2}[form], N, inst])
    return tuple(_subsystem(rng, form, N) for _ in range(FORMS[form]["halves"]))


# ---------------------------------------------------------------------------------------------------------
# packing into the images of the LDS node arrays, and back
# ---------------------------------------------------------------------------------------------------------
def stage_matrices(sub, k):
    """Ht_k (ND x ND) and M_k (NP x ND) of a subsystem."""
    nxa, nu = sub["nxa"], sub["nu"]
    ny, ND, NP = nxa + nu, nxa + nu + 1, nxa + 1
    Ht = np.zeros((ND, ND))
    Ht[:ny, :ny], Ht[:ny, ny], Ht[ny, :ny], Ht[ny, ny] = sub["Hyy"][k], sub["g"][k], sub["g"][k], sub["h0"][k]
    M = np.zeros((NP, ND))
    M[:nxa, :nxa], M[:nxa, nxa:ny], M[:nxa, ny], M[nxa, ny] = sub["A"][k], sub["B"][k], sub["c"][k], 1.0
    return Ht, M


def terminal_value(sub):
    nxa = sub["nxa"]
    Pt = np.zeros((nxa + 1, nxa + 1))
    Pt[:nxa, :nxa], Pt[:nxa, nxa], Pt[nxa, :nxa], Pt[nxa, nxa] = sub["PN"], sub["pN"], sub["pN"], sub["cN"]
    return Pt


def zi_of_p(p, nxa, ND):
    return p if p < nxa else ND - 1


def pack(form, waves, subs):
    """(M, H, G, dx0) images: M[slot][j][m] = M_k(m, j) with column stride NC, H and G packed symmetric, G[slot N]
    the terminal surrogate (Pt_N on the value indices, Quu = I, Gzu = 0); slot = nmaxs * half + k."""
    lay = layout(form, waves)
    nxa, nu, ND, NP, NC = lay["nxa"], lay["nu"], lay["ND"], lay["NP"], lay["NC"]
    Mi, Hi, Gi = np.zeros(lay["msize"]), np.zeros(lay["gsize"]), np.zeros(lay["gsize"])
    for h, sub in enumerate(subs):
        N = sub["N"]
        assert N + 1 <= lay["nmaxs"]
        for k in range(N):
            Ht, M = stage_matrices(sub, k)
            s = lay["nmaxs"] * h + k
            for j in range(ND):
                Mi[s * lay["swm"] + j * NC:s * lay["swm"] + j * NC + NP] = M[:, j]
            for i in range(ND):
                for j in range(i + 1):
                    Hi[s * lay["swg"] + hp(i, j)] = Ht[i, j]
        s = lay["nmaxs"] * h + N
        Pt = terminal_value(sub)
        for p in range(NP):
            for q in range(p + 1):
                Gi[s * lay["swg"] + hp(zi_of_p(p, nxa, ND), zi_of_p(q, nxa, ND))] = Pt[p, q]
        for a in range(nu):
            Gi[s * lay["swg"] + hp(nxa + a, nxa + a)] = 1.0
    return Mi, Hi, Gi, np.concatenate([sub["dx0"] for sub in subs])


def unpack_g(form, waves, Gimg, slot):
    """The ND x ND matrix G of a node slot (longdouble)."""
    lay = layout(form, waves)
    ND = lay["ND"]
    G = np.zeros((ND, ND), LD)
    for i in range(ND):
        for j in range(ND):
            G[i, j] = Gimg[slot * lay["swg"] + hp(i, j)]
    return G


def value_of_g(G, nxa, nu):
    """Pt (NP x NP): the Schur complement of G on the u block, over the value indices [x; 1]."""
    ND = nxa + nu + 1
    v = list(range(nxa)) + [ND - 1]
    u = list(range(nxa, nxa + nu))
    Quu = G[np.ix_(u, u)].astype(np.float64)
    Gzu = G[np.ix_(v, u)]
    X = np.linalg.solve(Quu, Gzu.T.astype(np.float64)).astype(LD)
    # one refinement step in longdouble
    X = X + np.linalg.solve(Quu, (Gzu.T - G[np.ix_(u, u)] @ X).astype(np.float64)).astype(LD)
    return G[np.ix_(v, v)] - Gzu @ X


# ---------------------------------------------------------------------------------------------------------
# reference 1: the dense KKT system, refined with longdouble residuals
# ---------------------------------------------------------------------------------------------------------
def kkt_system(sub):
    """K, b0 and the index maps: unknowns [x_0..x_N, u_0..u_{N-1}, lam_0..lam_N]; b depends on dx0 linearly."""
    N, nxa, nu = sub["N"], sub["nxa"], sub["nu"]
    nx, nuu = (N + 1) * nxa, N * nu
    n = 2 * nx + nuu
    K, b = np.zeros((n, n)), np.zeros(n)
    X = lambda k: slice(k * nxa, (k + 1) * nxa)
    U = lambda k: slice(nx + k * nu, nx + (k + 1) * nu)
    Lm = lambda k: slice(nx + nuu + k * nxa, nx + nuu + (k + 1) * nxa)
    for k in range(N):
        Hyy, g = sub["Hyy"][k], sub["g"][k]
        K[X(k), X(k)] += Hyy[:nxa, :nxa]; K[X(k), U(k)] += Hyy[:nxa, nxa:]
        K[U(k), X(k)] += Hyy[nxa:, :nxa]; K[U(k), U(k)] += Hyy[nxa:, nxa:]
        b[X(k)] -= g[:nxa]; b[U(k)] -= g[nxa:]
        # x_{k+1} - A x_k - B u_k = c_k, multiplier lam_{k+1}
        K[Lm(k + 1), X(k + 1)] += np.eye(nxa); K[Lm(k + 1), X(k)] -= sub["A"][k]; K[Lm(k + 1), U(k)] -= sub["B"][k]
        b[Lm(k + 1)] = sub["c"][k]
    K[X(N), X(N)] += sub["PN"]; b[X(N)] -= sub["pN"]
    K[Lm(0), X(0)] += np.eye(nxa)               # x_0 = dx0, multiplier lam_0
    c0 = nx + nuu
    K[:c0, c0:] = K[c0:, :c0].T
    return K, b, X, U, Lm


def refined_solve(K, B):
    """K X = B (B [n, m]) in float64, refined with longdouble residuals until the residual stops shrinking.
    Returns X (longdouble) and the relative residual max|K X - B| / (|K| |X| + |B|) (infinity norms)."""
    Kl, Bl = K.astype(LD), np.asarray(B, np.float64).astype(LD)
    Kinv = np.linalg.inv(K)
    X = (Kinv @ B).astype(LD)
    res = lambda X: Bl - Kl @ X
    r = res(X)
    best = np.max(np.abs(r))
    for _ in range(20):
        Xn = X + (Kinv @ r.astype(np.float64)).astype(LD)
        rn = res(Xn)
        if np.max(np.abs(rn)) >= best:
            break
        X, r, best = Xn, rn, np.max(np.abs(rn))
    scale = np.max(np.sum(np.abs(Kl), axis=1)) * np.max(np.abs(X)) + np.max(np.abs(Bl))
    return X, float(best / scale)


@functools.lru_cache(maxsize=None)
def dense_reference(form, N, inst, half=0, override=None):
    """dx [N+1, nxa], du [N, nu], lam [N+1, nxa] (longdouble), Pt_0 (NP x NP) and the relative KKT residual."""
    sub = problem(form, N, inst)[half]
    nxa, nu = sub["nxa"], sub["nu"]
    K, b, X, U, Lm = kkt_system(sub)
    # right-hand sides: dx0, then x_0 = 0 and x_0 = e_i for the value function of node 0
    B = np.tile(b[:, None], (1, nxa + 2))
    B[Lm(0), 0] = sub["dx0"]
    for i in range(nxa):
        B[Lm(0), 2 + i][i] = 1.0
    S, resid = refined_solve(K, B)
    sol = S[:, 0]
    dx = np.array([sol[X(k)] for k in range(N + 1)])
    du = np.array([sol[U(k)] for k in range(N)])
    lam = np.array([sol[Lm(k)] for k in range(N + 1)])
    # Pt_0: lam_0 = -(P x_0 + p); the corner is twice the optimal cost from x_0 = 0
    Pt = np.zeros((nxa + 1, nxa + 1), LD)
    l0 = S[Lm(0), 1]
    Pt[:nxa, nxa] = Pt[nxa, :nxa] = -l0
    for i in range(nxa):
        Pt[:nxa, i] = -(S[Lm(0), 2 + i] - l0)
    z = S[:, 1]
    cost = LD(sub["cN"]) / 2
    for k in range(N):
        y = np.concatenate([z[X(k)], z[U(k)]])
        cost += y @ (sub["Hyy"][k].astype(LD) @ y) / 2 + sub["g"][k].astype(LD) @ y + LD(sub["h0"][k]) / 2
    xN = z[X(N)]
    cost += xN @ (sub["PN"].astype(LD) @ xN) / 2 + sub["pN"].astype(LD) @ xN
    Pt[nxa, nxa] = 2 * cost
    return dict(dx=dx, du=du, lam=lam, Pt0=Pt, resid=resid)


# ---------------------------------------------------------------------------------------------------------
# reference 2: the textbook recursion in float64 (sets the tolerance only)
# ---------------------------------------------------------------------------------------------------------
def textbook_recursion(sub):
    N, nxa = sub["N"], sub["nxa"]
    P, p = [None] * (N + 1), [None] * (N + 1)
    Kg, kf, Quu = [None] * N, [None] * N, [None] * N
    P[N], p[N] = sub["PN"].copy(), sub["pN"].copy()
    for k in range(N - 1, -1, -1):
        A, B, c, H, g = sub["A"][k], sub["B"][k], sub["c"][k], sub["Hyy"][k], sub["g"][k]
        w = P[k + 1] @ c + p[k + 1]
        Qxx = H[:nxa, :nxa] + A.T @ P[k + 1] @ A
        Qux = H[nxa:, :nxa] + B.T @ P[k + 1] @ A
        Quu[k] = H[nxa:, nxa:] + B.T @ P[k + 1] @ B
        qx, qu = g[:nxa] + A.T @ w, g[nxa:] + B.T @ w
        Kg[k], kf[k] = -np.linalg.solve(Quu[k], Qux), -np.linalg.solve(Quu[k], qu)
        P[k] = Qxx + Qux.T @ Kg[k]
        P[k] = (P[k] + P[k].T) / 2
        p[k] = qx + Qux.T @ kf[k]
    dx, du, lam = np.zeros((N + 1, nxa)), np.zeros((N, sub["nu"])), np.zeros((N + 1, nxa))
    dx[0] = sub["dx0"]
    for k in range(N):
        du[k] = Kg[k] @ dx[k] + kf[k]
        dx[k + 1] = sub["A"][k] @ dx[k] + sub["B"][k] @ du[k] + sub["c"][k]
    for k in range(N + 1):
        lam[k] = -(P[k] @ dx[k] + p[k])
    return dict(dx=dx, du=du, lam=lam, Quu=Quu, P=P)


def rel_err(got, ref):
    """Largest error of each of dx, du, lam over all nodes, scaled by the quantity's infinity norm over the
    horizon; the largest of the three."""
    out = 0.0
    for q in ("dx", "du", "lam"):
        r = np.asarray(ref[q], LD)
        out = max(out, float(np.max(np.abs(np.asarray(got[q], LD) - r)) / np.max(np.abs(r))))
    return out


@functools.lru_cache(maxsize=None)
def e_ref(form, N):
    """Distance of the float64 textbook recursion from the refined dense solution, the largest over the shape's
    instances and subsystems."""
    e = 0.0
    for inst in range(INSTANCES):
        for half, sub in enumerate(problem(form, N, inst)):
            e = max(e, rel_err(textbook_recursion(sub), dense_reference(form, N, inst, half)))
    return e


def tolerance(form, N):
    """16 e_ref (the engine's other summation order, frcp's 4e-16 against a division), floor 64 x 2^-53."""
    return max(16.0 * e_ref(form, N), 64.0 * 2.0 ** -53)


# ---------------------------------------------------------------------------------------------------------
# inertia: one stage's Huu lowered until the reference Quu of that node is negative definite
# ---------------------------------------------------------------------------------------------------------
def with_negative_quu(sub, node):
    """A copy of the subsystem whose Quu at ``node`` is the original minus 1.5 times its largest eigenvalue:
    every eigenvalue is below -0.5 lambda_max, far from a rounding question."""
    Quu = textbook_recursion(sub)["Quu"][node]
    shift = 1.5 * float(np.max(np.linalg.eigvalsh(Quu)))
    out = dict(sub)
    out["Hyy"] = sub["Hyy"].copy()
    nxa = sub["nxa"]
    out["Hyy"][node, nxa:, nxa:] -= shift * np.eye(sub["nu"])
    return out


def flag_nodes(N):
    return sorted({0, N // 2, N - 1} | ({32} if N > 33 else set()))
