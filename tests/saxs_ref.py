"""References of the SAXS tests (tests/test_saxs.py, tests/test_saxs_host.py): the Debye sum in float64 numpy, the float32
restatement of the sequence include/codlad_hip.h states for codlad_saxs_debye - the same reduction constants, polynomial,
series branch, fp32 runs and float64 order - and the seeded cases.  Every array a case hands out is read-only."""
import functools
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def header_constants():
    """Every CODLAD_SAXS_* of the header: hex floats as float32, the rest as int."""
    text = open(os.path.join(ROOT, "include", "codlad_hip.h")).read()
    out = {}
    for name, value in re.findall(r"#define CODLAD_SAXS_(\w+) (\S+)", text):
        out[name] = F(float.fromhex(value[:-1])) if "p" in value else int(value)
    return out


K = header_constants()
CHUNK, MAX_Q, MAX_TYPES = K["Q_CHUNK"], K["MAX_Q"], K["MAX_TYPES"]
X_MAX, X_SMALL, SIN_ULPS = float(K["X_MAX"]), float(K["X_SMALL"]), K["SIN_ULPS"]
LANES, WAVES = 64, 4


# ------------------------------------------------------------------------------------------------ the restatement --
def sin32(x):
    """The header's sine of a float32 array x >= 0: float32 operations only, one rounding each."""
    x = np.asarray(x, dtype=F)
    with np.errstate(invalid="ignore", over="ignore"):
        kf = np.rint(x * K["INV_PI"])
        y = ((x - kf * K["P1"]) - kf * K["P2"]) - kf * K["P3"]
        s = y * y
        p = K["S11"] * s + K["S9"]
        p = p * s + K["S7"]
        p = p * s + K["S5"]
        p = p * s + K["S3"]
        v = y + (y * s) * p
        odd = (np.nan_to_num(kf, nan=0.0, posinf=0.0).astype(np.int64) & 1).astype(np.uint32) << np.uint32(31)
    assert v.dtype == F
    return (v.view(np.uint32) ^ odd).view(F)


def sinc32(x, inv_r, inv_q):
    """sinc of x = q * r as the header selects it: the series below X_SMALL, (sin * inv_r) * inv_q from there on."""
    with np.errstate(invalid="ignore", over="ignore"):
        far = (sin32(x) * inv_r) * inv_q
        x2 = x * x
        series = F(1) - (x2 * K["C6"]) * (F(1) - x2 * K["C20"])
    assert far.dtype == F and series.dtype == F
    return np.where(x < K["X_SMALL"], series, far)


def debye32(x, types, ff, q):
    """The kernel's own arithmetic for one structure x float32 [n, 3] -> I float64 [Q]."""
    x, ff, q = np.asarray(x, dtype=F), np.asarray(ff, dtype=F), np.asarray(q, dtype=F)
    types = np.asarray(types)
    n, Q = x.shape[0], q.shape[0]
    B = (n + LANES - 1) // LANES
    P = (B + 1) // 2
    with np.errstate(divide="ignore"):
        iq = F(1) / q
    lanes = np.arange(LANES)
    partial = np.zeros((P, Q))
    for c0 in range(0, Q, CHUNK):
        ks = slice(c0, min(c0 + CHUNK, Q))
        kc = ks.stop - ks.start
        for p in range(P):
            E = np.zeros((WAVES, LANES, kc))
            for rb in ((p,) if B - 1 - p == p else (p, B - 1 - p)):
                i = rb * LANES + lanes
                ic = np.minimum(i, n - 1)
                xi = x[ic]
                fi = np.where((i < n)[:, None], ff[types[ic], ks], F(0)).astype(np.float64)
                for w in range(WAVES):
                    D = np.zeros((LANES, kc))
                    for t in range(rb + w, B, WAVES):
                        j = np.arange(t * LANES, min(t * LANES + LANES, n))
                        d = x[j][None, :, :] - xi[:, None, :]
                        r = np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])
                        with np.errstate(divide="ignore"):
                            inv_r = F(1) / r
                        xx = q[ks][None, None, :] * r[:, :, None]
                        term = ff[types[j], ks][None, :, :] * sinc32(xx, inv_r[:, :, None], iq[ks][None, None, :])
                        term = np.where((j[None, :] > i[:, None])[:, :, None], term, F(0))
                        assert term.dtype == F
                        acc = np.zeros((LANES, kc), dtype=F)
                        for jj in range(j.shape[0]):
                            acc = acc + term[:, jj, :]
                        D = D + acc.astype(np.float64)
                    E[w] = E[w] + (2.0 * (fi * D) + (fi * fi if w == 0 else 0.0))
            for st in (32, 16, 8, 4, 2, 1):
                E = E + E[:, lanes ^ st, :]
            partial[p, ks] = ((E[0, 0] + E[1, 0]) + E[2, 0]) + E[3, 0]
    I = np.zeros(Q)
    for p in range(P):
        I = I + partial[p]
    return I


# ------------------------------------------------------------------------------------------------- the reference --
def debye64(x, types, ff, q):
    """Float64 throughout, from the float32 inputs the kernel reads: x [S, n, 3] -> (I [S, Q], A [S, Q]) with
    A = sum_i f_i^2 + 2 sum_{i<j} |f_i f_j sinc|, the scale of the rounding errors of the sum."""
    x = np.asarray(x, dtype=F).astype(np.float64)
    f = np.asarray(ff, dtype=F).astype(np.float64)[np.asarray(types)]                 # [n, Q]
    q = np.asarray(q, dtype=F).astype(np.float64)
    n = x.shape[1]
    iu = np.triu_indices(n, 1)
    I, A = np.empty((x.shape[0], q.shape[0])), np.empty((x.shape[0], q.shape[0]))
    self_term = (f * f).sum(0)
    ff_pair = f[iu[0]] * f[iu[1]]                                                     # [pairs, Q]
    for s in range(x.shape[0]):
        d = x[s][iu[1]] - x[s][iu[0]]
        xr = np.sqrt((d * d).sum(1))[:, None] * q[None, :]
        with np.errstate(invalid="ignore", divide="ignore"):
            sinc = np.where(xr == 0.0, 1.0, np.sin(xr) / xr)
        I[s] = self_term + 2.0 * (ff_pair * sinc).sum(0)
        A[s] = self_term + 2.0 * np.abs(ff_pair * sinc).sum(0)
    return I, A


# ------------------------------------------------------------------------------------------------------ the cases --
SIZES = (1, 2, 63, 64, 65, 129, 300)          # tile edges; 129 and 300 have an odd middle block of the pairing (B = 3, 5)
Q_SIZES = (1, CHUNK, CHUNK + 1, 51)
T_SIZES = (1, 5, MAX_TYPES)
SHIFTS = (0.0, 500.0)
N_STRUCT = 3


def case_keys():
    """(n, Q, T, shift, kind): every size with the usual grid at both shifts, every Q and T at the tile edges, and the three
    special inputs - two coincident atoms, q[0] = 0, and an extent that takes q * r past several thousand radians."""
    keys = [(n, 51, 5, 0.0, "plain") for n in SIZES] + [(n, CHUNK + 1, 5, 500.0, "plain") for n in SIZES]
    keys += [(65, 1, 1, 0.0, "plain"), (63, 1, MAX_TYPES, 500.0, "plain"), (64, CHUNK, 1, 500.0, "plain"),
             (129, CHUNK, MAX_TYPES, 0.0, "plain"), (300, CHUNK, MAX_TYPES, 500.0, "plain"), (2, 1, 1, 500.0, "plain")]
    keys += [(65, 51, 5, 0.0, "coincident"), (129, CHUNK + 1, 5, 500.0, "q0"), (65, CHUNK + 1, 5, 0.0, "far")]
    return keys


def case_id(key):
    return f"n{key[0]}-Q{key[1]}-T{key[2]}-{'shifted' if key[3] else 'origin'}-{key[4]}"


def _freeze(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def case(key):
    """x float32 [3, n, 3], types int32 [n], ff float32 [T, Q], q float32 [Q] of a key, its float64 reference I, A, the
    restatement's I32 and dev32 = max |I32 - I| / A."""
    n, Q, T, shift, kind = key
    rng = np.random.default_rng(1000003 * n + 101 * Q + 7 * T + int(shift) + len(kind))
    extent = 1400.0 if kind == "far" else 4.0 * max(n, 2) ** (1.0 / 3.0)              # a protein's density, roughly
    x = (rng.uniform(-0.5, 0.5, (N_STRUCT, n, 3)) * extent + shift).astype(F)
    if kind == "coincident":
        x[:, 40] = x[:, 7]
        x[1, 64] = x[1, 0]                                                             # across a tile edge too
    q_hi = 10.0 if kind == "far" else 0.5
    q = np.linspace(0.0 if kind == "q0" else 0.01, q_hi, Q).astype(F) if Q > 1 else np.array([0.0 if kind == "q0" else 0.2], dtype=F)
    types = rng.integers(0, T, n).astype(np.int32)
    if n >= T:
        types[:T] = np.arange(T)                                                       # every type occurs
    # form factors of the usual size and shape: positive, falling with q, some types negative (below the solvent)
    f0 = rng.uniform(-2.0, 9.0, T)
    width = rng.uniform(5.0, 40.0, T)
    ff = (f0[:, None] * np.exp(-width[:, None] * (q.astype(np.float64)[None, :] / (4 * np.pi)) ** 2)).astype(F)
    I, A = debye64(x, types, ff, q)
    I32 = np.stack([debye32(x[s], types, ff, q) for s in range(N_STRUCT)])
    dev32 = float((np.abs(I32 - I) / A).max())
    return _freeze(dict(x=x, types=types, ff=ff, q=q, I=I, A=A, I32=I32, dev32=dev32))


def two_atoms(f1, f2, r, q):
    """The analytic curve of two atoms r apart, float64."""
    q = np.asarray(q, dtype=np.float64)
    xr = q * r
    with np.errstate(invalid="ignore", divide="ignore"):
        sinc = np.where(xr == 0.0, 1.0, np.sin(xr) / xr)
    return f1 * f1 + f2 * f2 + 2.0 * f1 * f2 * sinc
