"""Finds the rigid transforms frozen as DOCK in tests/dssp_ref.py: the second of two ideal 7-residue strands is moved
onto the first so that exactly the wanted Kabsch-Sander bonds of an antiparallel / a parallel ladder form.

    python tools/dssp_dock_search.py [anti|par] [--seed N]

CPU only, float64, against tests/dssp_ref.stage1.  A hill climb over the six rigid parameters (rotation vector, shift);
every climb starts at or near the least-squares fit that puts each wanted acceptor O 2.9 A along its donor's N-H.
Objective: the energy of the wanted pairs clipped at -2.5 kcal/mol (so that no pair is rewarded for a clash), a quadratic
pull of their O..N distances towards 2.9 A and a penalty on backbone atoms of the two strands closer than 3 A.  A result is
accepted when the bond matrix is exactly the wanted one plus the bonds each strand has with itself before docking; it
prints the constants and the smallest |E + 0.5| over all eligible pairs.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from tests import dssp_ref as dr                                                                     # noqa: E402


def score(kind, params, top, bb, res_kind, heavy, own=frozenset()):
    _top, x = dr.strands(kind, dock=(params[:3], params[3:]))
    r = dr.stage1(x, bb, res_kind)
    en = r["energy"][0]
    want = dr.DOCK_BONDS[kind]
    val = 0.0
    for i, j in want:
        e = en[i, j]
        d = np.linalg.norm(x[top.atom(i, "O")] - x[top.atom(j, "N")])
        val += (max(e, -2.5) if np.isfinite(e) else 0.0) + 0.5 * (d - 2.9) ** 2
    a, b = x[heavy[0]], x[heavy[1]]
    d = np.sqrt(((a[:, None] - b[None]) ** 2).sum(-1))
    val += 5.0 * (np.clip(3.0 - d, 0.0, None) ** 2).sum()
    exact = set(zip(*np.nonzero(r["hb"][0]))) == set(want) | own
    with np.errstate(invalid="ignore"):
        margin = np.nanmin(np.abs(en - dr.E_BOND))
    return val, exact, margin


def fitted_start(kind, top, x):
    """The transform that puts every wanted acceptor O on the point 2.9 A along its donor's N-H: a least-squares fit of
    the second strand's points onto the first's (Kabsch).  Every climb starts at or near it."""
    n = top.n_residues // 2
    h = {}
    for j in range(1, 2 * n):
        if j != n:
            d = x[top.atom(j - 1, "C")] - x[top.atom(j - 1, "O")]
            h[j] = d / np.linalg.norm(d)
    fixed, moving = [], []
    for i, j in dr.DOCK_BONDS[kind]:
        o, q = x[top.atom(i, "O")], x[top.atom(j, "N")] + 2.9 * h[j]
        (fixed if i < n else moving).append(o)
        (moving if i < n else fixed).append(q)
    fixed, moving = np.array(fixed), np.array(moving)
    cf, cm = fixed.mean(0), moving.mean(0)
    u, _s, vt = np.linalg.svd((moving - cm).T @ (fixed - cf))
    d = np.sign(np.linalg.det(vt.T @ u.T))
    rot = vt.T @ np.diag([1.0, 1.0, d]) @ u.T
    angle = np.arccos(np.clip((np.trace(rot) - 1) / 2, -1, 1))
    axis = np.array([rot[2, 1] - rot[1, 2], rot[0, 2] - rot[2, 0], rot[1, 0] - rot[0, 1]])
    rotvec = axis / np.linalg.norm(axis) * angle
    return np.concatenate([rotvec, cf - dr.rotation(rotvec) @ cm])


def search(kind, seed, starts=20, steps=600):
    rng = np.random.default_rng(seed)
    top, x0 = dr.strands(kind, dock=((0, 0, 0), (0, 0, 0)))
    bb, res_kind = dr.tables(top)
    n = top.n_residues // 2
    names = ("N", "CA", "C", "O", "CB")
    heavy = ([top.atom(r, a) for r in range(n) for a in names], [top.atom(r, a) for r in range(n, 2 * n) for a in names])
    p0 = fitted_start(kind, top, x0)
    # the bonds a strand has with itself before docking (i -> i + 2 at (-119, 113): no turn, no bridge) stay
    own = frozenset(zip(*np.nonzero(dr.stage1(x0, bb, res_kind)["hb"][0])))
    best = None
    for k in range(starts):
        p = p0 + (rng.normal(size=6) * np.array([0.05] * 3 + [0.3] * 3) if k else 0.0)
        val, exact, margin = score(kind, p, top, bb, res_kind, heavy, own)
        step = np.array([0.05] * 3 + [0.3] * 3)
        for _it in range(steps):
            q = p + rng.normal(size=6) * step
            v, ex, mg = score(kind, q, top, bb, res_kind, heavy, own)
            if v < val:
                p, val, exact, margin = q, v, ex, mg
                step *= 1.1
            else:
                step *= 0.98
        print(f"start {k}: objective {val:.3f} exact {exact} margin {margin:.4f}", flush=True)
        if exact and (best is None or margin > best[2]):
            best = (p, val, margin)
            if margin > 0.04:
                break
    return best


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("kind", nargs="?", choices=("anti", "par"))
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    for kind in ([args.kind] if args.kind else ["anti", "par"]):
        found = search(kind, args.seed)
        if found is None:
            print(kind, "no exact ladder found; try another --seed")
            continue
        p, val, margin = found
        p = [float(v) for v in p]
        print(f'    "{kind}": (({p[0]!r}, {p[1]!r}, {p[2]!r}), ({p[3]!r}, {p[4]!r}, {p[5]!r})),'
              f"   # objective {val:.3f}, min |E + 0.5| {margin:.4f}")
