"""References of the SAXS hydration tests (tests/test_saxs_hydration.py, tests/test_saxs_hydration_host.py): the six partial
Debye sums in float64 numpy, the float32 restatement of the sequence include/codlad_hip.h states for codlad_saxs_partials
(the sine and the selection of sinc are tests/saxs_ref.py's), the combination and the grid fit in the stated float64
order, the direct double sum of |F|^2, and the seeded cases.  Every array a case hands out is read-only."""
import functools

import numpy as np

from tests import saxs_ref as sr

F = np.float32
K = sr.header_constants()
CHUNK, MAX_GRID, N_PARTIALS = K["HYD_Q_CHUNK"], K["HYD_MAX_GRID"], K["HYD_PARTIALS"]
LANES, WAVES = sr.LANES, sr.WAVES
NAMES = ("tt", "td", "dd", "ts", "ds", "ss")
PAIRS = ((0, 0), (0, 1), (1, 1), (0, 2), (1, 2), (2, 2))          # a partial's two factors among (t, d, s)
R_M = 1.62


# ------------------------------------------------------------------------------------------------- the reference --
def _sinc64(x, q):
    """sinc(q r_ij) of every pair i < j of one float64 structure -> (iu, sinc [pairs, Q])."""
    iu = np.triu_indices(x.shape[0], 1)
    d = x[iu[1]] - x[iu[0]]
    xr = np.sqrt((d * d).sum(1))[:, None] * q[None, :]
    with np.errstate(invalid="ignore", divide="ignore"):
        return iu, np.where(xr == 0.0, 1.0, np.sin(xr) / xr)


def _factors64(types, ff_t, ff_d, weight_s, Q):
    t = np.asarray(ff_t, dtype=F).astype(np.float64)[np.asarray(types)]
    d = np.asarray(ff_d, dtype=F).astype(np.float64)[np.asarray(types)]
    s = np.repeat(np.asarray(weight_s, dtype=F).astype(np.float64)[:, None], Q, axis=1)
    return t, d, s


def partials64(x, types, ff_t, ff_d, weight, q):
    """Float64 throughout, from the float32 inputs the kernel reads: x [S, n, 3], weight [S, n] -> (P [S, 6, Q], A [S, 6, Q])
    with P_ab = sum_i a_i b_i + sum_{i<j} (a_i b_j + b_i a_j) sinc and A_ab the same sum of absolute values, the scale of
    its rounding errors."""
    x = np.asarray(x, dtype=F).astype(np.float64)
    q = np.asarray(q, dtype=F).astype(np.float64)
    S, Q = x.shape[0], q.shape[0]
    P, A = np.empty((S, 6, Q)), np.empty((S, 6, Q))
    for s in range(S):
        f = _factors64(types, ff_t, ff_d, weight[s], Q)
        iu, sinc = _sinc64(x[s], q)
        for c, (a, b) in enumerate(PAIRS):
            fa, fb = f[a], f[b]
            P[s, c] = (fa * fb).sum(0) + ((fa[iu[0]] * fb[iu[1]] + fb[iu[0]] * fa[iu[1]]) * sinc).sum(0)
            A[s, c] = np.abs(fa * fb).sum(0) + ((np.abs(fa[iu[0]] * fb[iu[1]]) + np.abs(fb[iu[0]] * fa[iu[1]])) * np.abs(sinc)).sum(0)
    return P, A


def expansion64(q, c1, r_m=R_M):
    """G(q, c1) = c1^3 exp(-(4 pi / 3)^(3/2) q^2 r_m^2 (c1^2 - 1) / (4 pi)) -> float64 [len(c1), Q]."""
    q = np.asarray(q, dtype=np.float64).reshape(1, -1)
    c1 = np.asarray(c1, dtype=np.float64).reshape(-1, 1)
    return c1 ** 3 * np.exp(-((4.0 * np.pi / 3.0) ** 1.5 * q * q * float(r_m) ** 2 * (c1 * c1 - 1.0)) / (4.0 * np.pi))


def coefficients64(q, water, c1, c2, r_m=R_M):
    """The six coefficients of the combination at one (c1, c2) -> float64 [6, Q]."""
    u = 1.0 - expansion64(q, [c1], r_m)[0]
    w = float(c2) * np.asarray(water, dtype=np.float64)
    return np.stack([np.ones_like(u), 2.0 * u, u * u, 2.0 * w, (2.0 * w) * u, w * w])


def _combine(P, G, fw, c2):
    """The header's order; P [..., 6, Q], G and c2 broadcast against [..., Q]."""
    u, w = 1.0 - G, c2 * fw
    I = P[..., 0, :] + (2.0 * u) * P[..., 1, :]
    I = I + (u * u) * P[..., 2, :]
    I = I + (2.0 * w) * P[..., 3, :]
    I = I + ((2.0 * w) * u) * P[..., 4, :]
    return I + (w * w) * P[..., 5, :]


def combine64(P, q, water, c1, c2, r_m=R_M):
    """I(q; c1, c2) of P [..., 6, Q] in the float64 order the header states -> [..., Q]."""
    return _combine(np.asarray(P, dtype=np.float64), expansion64(q, [c1], r_m)[0], np.asarray(water, dtype=np.float64), float(c2))


def fit64(P, q, water, I_exp, sigma, c1, c2, r_m=R_M):
    """The grid fit of ONE curve set P [6, Q] in the stated order: sums over k ascending, the smallest chi2, the lowest flat
    index of a tie, a chi2 that is not finite never wins -> dict(chi2_grid, scale_grid [n1, n2], index, I)."""
    P = np.asarray(P, dtype=np.float64)
    c1, c2 = np.asarray(c1, dtype=np.float64).reshape(-1), np.asarray(c2, dtype=np.float64).reshape(-1)
    fw, exp, sig = (np.asarray(a, dtype=np.float64).reshape(-1) for a in (water, I_exp, sigma))
    G = expansion64(q, c1, r_m)
    Q = P.shape[-1]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        I = _combine(P[None, None], G[:, None, :], fw[None, None, :], c2[None, :, None])          # [n1, n2, Q]
        num, den = np.zeros(I.shape[:2]), np.zeros(I.shape[:2])
        for k in range(Q):
            wk = 1.0 / (sig[k] * sig[k])
            num = num + (exp[k] * I[:, :, k]) * wk
            den = den + (I[:, :, k] * I[:, :, k]) * wk
        scale = num / den
        total = np.zeros(I.shape[:2])
        for k in range(Q):
            r = (scale * I[:, :, k] - exp[k]) / sig[k]
            total = total + r * r
        chi2 = total / float(Q - 1)
    flat = chi2.reshape(-1)
    ok = np.isfinite(flat)
    index = int(np.argmin(np.where(ok, flat, np.inf))) if ok.any() else -1                     # argmin: the first of a tie
    best = I.reshape(-1, Q)[index] if index >= 0 else np.full(Q, np.nan)
    return dict(chi2_grid=chi2, scale_grid=scale, index=index, I=best)


def direct64(x, types, ff_t, ff_d, weight, q, water, c1, c2, r_m=R_M):
    """The double sum itself, float64: I = sum_i F_i^2 + 2 sum_{i<j} F_i F_j sinc with F = t + (1 - G) d + c2 f_w s."""
    x = np.asarray(x, dtype=F).astype(np.float64)
    q32 = np.asarray(q, dtype=F).astype(np.float64)
    u = 1.0 - expansion64(q, [c1], r_m)[0]
    w = float(c2) * np.asarray(water, dtype=np.float64)
    out = np.empty((x.shape[0], q32.shape[0]))
    for s in range(x.shape[0]):
        t, d, sw = _factors64(types, ff_t, ff_d, weight[s], q32.shape[0])
        Fi = t + u[None, :] * d + w[None, :] * sw
        iu, sinc = _sinc64(x[s], q32)
        out[s] = (Fi * Fi).sum(0) + 2.0 * (Fi[iu[0]] * Fi[iu[1]] * sinc).sum(0)
    return out


# ------------------------------------------------------------------------------------------------ the restatement --
def partials32(x, types, ff_t, ff_d, weight_s, q):
    """The kernel's own arithmetic for one structure x float32 [n, 3], weight_s float32 [n] -> P float64 [6, Q]."""
    x, q = np.asarray(x, dtype=F), np.asarray(q, dtype=F)
    tab = (np.asarray(ff_t, dtype=F), np.asarray(ff_d, dtype=F))
    wt = np.asarray(weight_s, dtype=F)
    types = np.asarray(types)
    n, Q = x.shape[0], q.shape[0]
    B = (n + LANES - 1) // LANES
    NW = (B + 1) // 2
    with np.errstate(divide="ignore"):
        iq = F(1) / q
    lanes = np.arange(LANES)
    partial = np.zeros((NW, 6, Q))
    for c0 in range(0, Q, CHUNK):
        ks = slice(c0, min(c0 + CHUNK, Q))
        kc = ks.stop - ks.start
        for p in range(NW):
            E = np.zeros((6, WAVES, LANES, kc))
            for rb in ((p,) if B - 1 - p == p else (p, B - 1 - p)):
                i = rb * LANES + lanes
                ic = np.minimum(i, n - 1)
                xi = x[ic]
                live = (i < n)[:, None]
                own = [np.where(live, tab[0][types[ic], ks], F(0)).astype(np.float64),
                       np.where(live, tab[1][types[ic], ks], F(0)).astype(np.float64),
                       np.where(live, wt[ic][:, None], F(0)).astype(np.float64) * np.ones((1, kc))]
                for w in range(WAVES):
                    D = np.zeros((3, LANES, kc))
                    for t in range(rb + w, B, WAVES):
                        j = np.arange(t * LANES, min(t * LANES + LANES, n))
                        d = x[j][None, :, :] - xi[:, None, :]
                        r = np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])
                        with np.errstate(divide="ignore"):
                            inv_r = F(1) / r
                        xx = q[ks][None, None, :] * r[:, :, None]
                        sinc = sr.sinc32(xx, inv_r[:, :, None], iq[ks][None, None, :])                # ONE sinc per (i, j, k)
                        pair = (j[None, :] > i[:, None])[:, :, None]
                        partner = (tab[0][types[j], ks][None, :, :], tab[1][types[j], ks][None, :, :], wt[j][None, :, None])
                        term = np.stack([np.where(pair, partner[v] * sinc, F(0)) for v in range(3)])    # t_j, d_j, s_j times sinc
                        assert term.dtype == F
                        acc = np.zeros((3, LANES, kc), dtype=F)
                        for jj in range(j.shape[0]):
                            acc = acc + term[:, :, jj, :]
                        D = D + acc.astype(np.float64)
                    for c, (a, b) in enumerate(PAIRS):
                        self_term = own[a] * own[b] if w == 0 else 0.0
                        if a == b:
                            E[c, w] = E[c, w] + (2.0 * (own[a] * D[a]) + self_term)
                        else:
                            E[c, w] = E[c, w] + ((own[a] * D[b] + own[b] * D[a]) + self_term)
            for st in (32, 16, 8, 4, 2, 1):
                E = E + E[:, :, lanes ^ st, :]
            partial[p, :, ks] = ((E[:, 0, 0] + E[:, 1, 0]) + E[:, 2, 0]) + E[:, 3, 0]
    P = np.zeros((6, Q))
    for p in range(NW):
        P = P + partial[p]
    return P


# ------------------------------------------------------------------------------------------------------ the cases --
SIZES = sr.SIZES                               # 1, 2, 63, 64, 65, 129, 300
Q_SIZES = (1, CHUNK, CHUNK + 1, 51)
T_SIZES = sr.T_SIZES
SHIFTS = sr.SHIFTS
N_STRUCT = sr.N_STRUCT
FIT_KEY = (300, 51, 5, 0.0, "plain")


def case_keys():
    """(n, Q, T, shift, kind): the combinations of saxs_ref.case_keys with this kernel's chunk."""
    keys = [(n, 51, 5, 0.0, "plain") for n in SIZES] + [(n, CHUNK + 1, 5, 500.0, "plain") for n in SIZES]
    keys += [(65, 1, 1, 0.0, "plain"), (63, 1, sr.MAX_TYPES, 500.0, "plain"), (64, CHUNK, 1, 500.0, "plain"),
             (129, CHUNK, sr.MAX_TYPES, 0.0, "plain"), (300, CHUNK, sr.MAX_TYPES, 500.0, "plain"), (2, 1, 1, 500.0, "plain")]
    keys += [(65, 51, 5, 0.0, "coincident"), (129, CHUNK + 1, 5, 500.0, "q0"), (65, CHUNK + 1, 5, 0.0, "far")]
    return keys


case_id = sr.case_id


def water_curve(q):
    """A shell water's form factor, roughly: positive and falling with q (float64)."""
    return 2.5 * np.exp(-12.0 * (np.asarray(q, dtype=np.float64) / (4 * np.pi)) ** 2)


@functools.lru_cache(maxsize=None)
def case(key):
    """x float32 [3, n, 3], types int32 [n], ff_t, ff_d float32 [T, Q], weight float32 [3, n], q float32 [Q], water float64 [Q]
    of a key; its float64 reference P, A [3, 6, Q], the restatement's P32 and dev32 [6] = max |P32 - P| / A per partial."""
    n, Q, T, shift, kind = key
    rng = np.random.default_rng(2000003 * n + 103 * Q + 11 * T + int(shift) + len(kind))
    extent = 1400.0 if kind == "far" else 4.0 * max(n, 2) ** (1.0 / 3.0)
    x = (rng.uniform(-0.5, 0.5, (N_STRUCT, n, 3)) * extent + shift).astype(F)
    if kind == "coincident":
        x[:, 40] = x[:, 7]
        x[1, 64] = x[1, 0]                                                             # across a tile edge too
    q_hi = 10.0 if kind == "far" else 0.5
    q = np.linspace(0.0 if kind == "q0" else 0.01, q_hi, Q).astype(F) if Q > 1 else np.array([0.0 if kind == "q0" else 0.2], dtype=F)
    types = rng.integers(0, T, n).astype(np.int32)
    if n >= T:
        types[:T] = np.arange(T)
    s2 = (q.astype(np.float64)[None, :] / (4 * np.pi)) ** 2
    # shaped like real form factors: t of either sign (a methyl lies below the solvent), d = density * volume * a Gaussian > 0
    t0 = rng.uniform(-2.0, 9.0, T)
    if T > 1:
        t0[0], t0[1] = -abs(t0[0]) - 0.5, abs(t0[1]) + 0.5                            # both signs in every table of two types or more
    ff_t = (t0[:, None] * np.exp(-rng.uniform(5.0, 40.0, T)[:, None] * s2)).astype(F)
    ff_d = (rng.uniform(1.0, 12.0, T)[:, None] * np.exp(-rng.uniform(20.0, 80.0, T)[:, None] * s2)).astype(F)
    # exposed fractions as 96 test points give them; about half of the atoms are buried
    weight = (rng.integers(0, 97, (N_STRUCT, n)) * (rng.uniform(0, 1, (N_STRUCT, n)) < 0.5)).astype(F) / F(96)
    P, A = partials64(x, types, ff_t, ff_d, weight, q)
    P32 = np.stack([partials32(x[s], types, ff_t, ff_d, weight[s], q) for s in range(N_STRUCT)])
    with np.errstate(invalid="ignore", divide="ignore"):
        dev32 = np.where(A > 0, np.abs(P32 - P) / A, 0.0).max(axis=(0, 2))
    return sr._freeze(dict(x=x, types=types, ff_t=ff_t, ff_d=ff_d, weight=weight, q=q, water=water_curve(q), P=P, A=A, P32=P32,
                           dev32=dev32))
