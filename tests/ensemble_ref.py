"""Host reference and inputs of the ensemble-analysis tests (tests/test_ensemble.py, tests/test_ensemble_host.py).

The reference is the SVD route in float64 numpy: centre, 3x3 covariance, singular values, sign(det) - the arithmetic of
`codlad_amd.metrics.superposed_rmsd`, which also yields e0 / n and the transform.  Inputs are built on the CPU in fp32
from fixed seeds; the reference of every case is computed once per session and never modified."""
import functools

import numpy as np

EPS = 2.0 ** -52
SIZES = (1, 2, 3, 4, 63, 64, 65, 255, 256, 257, 1000, 4099)
CATEGORIES = ("noisy", "rigid", "mirror", "unrelated", "planar", "collinear", "identical")
OFFSETS = (0.0, 1000.0)


def kabsch(a, b):
    """a, b [n, 3] (any float dtype) -> dict(msd, e0n = (Ga + Gb) / n, R [3, 3], t [3]) in float64, with a @ R.T + t
    superposed on b by the optimal PROPER rotation.  msd is not clamped at 0."""
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    n = a.shape[0]
    ca, cb = a.mean(0), b.mean(0)
    ac, bc = a - ca, b - cb
    cov = ac.T @ bc                                    # S[r][c] = sum a_r b_c
    u, sv, vt = np.linalg.svd(cov)
    d = np.sign(np.linalg.det(u @ vt))
    e0 = float((ac * ac).sum() + (bc * bc).sum())
    msd = (e0 - 2.0 * float(sv[0] + sv[1] + d * sv[2])) / n
    # maximise tr(R S): R = V diag(1, 1, d) U^T
    R = vt.T @ np.diag([1.0, 1.0, d if d != 0 else 1.0]) @ u.T
    if np.linalg.det(R) < 0:                           # d = 0 (a singular covariance): any proper completion
        R = vt.T @ np.diag([1.0, 1.0, -1.0]) @ u.T
    return {"msd": msd, "e0n": e0 / n, "R": R, "t": cb - R @ ca}


def msd_bound(n, e0n):
    """|msd_dev - max(msd_ref, 0)| <= (n + 16) 2^-52 e0 / n: n 2^-52 e0 / n is the worst-case error of an fp64 sum of n
    products (sum |a b| <= e0 / 2, twice for the factor 2 of the formula); the 16 covers the 4x4 eigen-solve against the
    SVD."""
    return (n + 16) * EPS * e0n


def plain_msd(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return float(((a - b) ** 2).sum(-1).mean())


def _rotation(rng):
    q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def make_pair(category, n, offset, seed):
    """-> (a, b) fp32 [n, 3]: a blob of spread 5 A placed `offset` A from the origin and its partner."""
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((n, 3)) * 5.0
    if category == "planar":
        a[:, 2] = 0.0
    elif category == "collinear":
        a = np.outer(rng.standard_normal(n) * 5.0, np.array([0.6, 0.0, 0.8]))
    shift = np.array([offset, -0.5 * offset, 0.25 * offset])
    if category == "noisy":
        b = a + 0.3 * rng.standard_normal((n, 3))
    elif category == "rigid":
        b = a @ _rotation(rng).T + np.array([1.5, -2.5, 3.5])
    elif category == "mirror":
        b = a * np.array([1.0, 1.0, -1.0])
    elif category == "unrelated":
        b = rng.standard_normal((n, 3)) * 5.0
    elif category in ("planar", "collinear"):
        # a rigidly moved, slightly noisy copy that stays in the plane / on the line
        noise = 0.3 * rng.standard_normal((n, 3))
        if category == "planar":
            noise[:, 2] = 0.0
            b = a + noise
        else:
            b = a + np.outer(noise[:, 0], np.array([0.6, 0.0, 0.8]))
    elif category == "identical":
        b = a.copy()
    else:
        raise KeyError(category)
    a32 = (a + shift).astype(np.float32)
    b32 = a32.copy() if category == "identical" else (b + shift).astype(np.float32)
    return a32, b32


def case_seed(category, n, offset):
    return 100003 * CATEGORIES.index(category) + 7 * n + (1 if offset else 0)


@functools.lru_cache(maxsize=None)
def cases_of_size(n):
    """Every category x offset at n atoms -> (labels, a [C, n, 3] fp32, b [C, n, 3] fp32, refs [C] of kabsch dicts)."""
    labels, aa, bb, refs = [], [], [], []
    for cat in CATEGORIES:
        for off in OFFSETS:
            a, b = make_pair(cat, n, off, case_seed(cat, n, off))
            labels.append((cat, off))
            aa.append(a)
            bb.append(b)
            refs.append(kabsch(a, b))
    a, b = np.stack(aa), np.stack(bb)
    a.setflags(write=False)
    b.setflags(write=False)
    return tuple(labels), a, b, tuple(refs)


@functools.lru_cache(maxsize=None)
def batch(P, n, seed):
    """P unrelated-ish pairs (noisy copies with growing noise) at n atoms, half of them far from the origin."""
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((P, n, 3)) * 5.0
    b = a + rng.standard_normal((P, n, 3)) * np.linspace(0.05, 3.0, P)[:, None, None]
    shift = np.where(np.arange(P) % 2 == 0, 0.0, 1000.0)[:, None, None]
    a32, b32 = (a + shift).astype(np.float32), (b + shift).astype(np.float32)
    a32.setflags(write=False)
    b32.setflags(write=False)
    return a32, b32
