"""Reference of lDDT (metrics.lddt, codlad_lddt): a plain numpy evaluation by atom NAME with a symmetry table of its own;
it shares no code with codlad_amd/metrics/lddt.py.

The same evaluation runs in float64 (the reference) and in float32 with one rounding per operation in the kernel's order
(the restatement: every decision of the kernel is `fl32 < fl32` on values made by that sequence, so the restatement's
integers are the kernel's).  `sandwich` brackets the float32 counts by float64 counts with every cut moved in, and out,
by a margin derived from the roundings of a float32 distance."""
import numpy as np

from tests import stereo_ref as sr

CUTOFF = 15.0
THRESHOLDS = (0.5, 1.0, 2.0, 4.0)
# the exchanges of a 180 degree flip, per residue type, as "A=B" pairs that go together
FLIPS = {"ARG": "NH1=NH2", "ASP": "OD1=OD2", "GLU": "OE1=OE2", "LEU": "CD1=CD2", "PHE": "CD1=CD2 CE1=CE2",
         "TYR": "CD1=CD2 CE1=CE2", "VAL": "CG1=CG2"}
# max |coordinate| * EPS_FACTOR bounds the error of a float32 distance: about 3 roundings of relative size 2^-24 on
# d <= 2 sqrt(3) max|x|, 3 * 2 sqrt(3) = 10.4 < 16
EPS_FACTOR = 16.0 * 2.0 ** -24
CAP = 2e-4                         # undecided decisions / ((T + 1) * sum(total)) a test case may have
CASES = ((60, 0.3), (60, 1.5), (129, 0.8))     # (residues, noise sigma in A) of planted(n, seed=7)


def distances(x, rows, dtype):
    """[len(rows), n]: sqrt((dx*dx + dy*dy) + dz*dz) in `dtype`, one rounding per operation."""
    x = np.asarray(x, dtype=dtype)
    d = x[rows][:, None, :] - x[None, :, :]
    return np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])


def counts(model, ref, res, dtype=np.float64, rows=None, cutoff=CUTOFF, thresholds=THRESHOLDS, seq_sep=1, margin=0.0):
    """(total [k], preserved [k, T]) int64 of the atoms `rows` (default all): partners j with |res_i - res_j| >= seq_sep and
    d_ref < cutoff + margin, and of those the ones with |d_mod - d_ref| < t + 2 * margin.  margin only in float64."""
    res = np.asarray(res)
    rows = np.arange(res.shape[0]) if rows is None else np.asarray(rows)
    d_ref, d_mod = distances(ref, rows, dtype), distances(model, rows, dtype)
    with np.errstate(invalid="ignore"):
        inc = (np.abs(res[rows][:, None] - res[None, :]) >= seq_sep) & (d_ref < dtype(cutoff) + dtype(margin))
        diff = np.abs(d_mod - d_ref)
        kept = np.stack([(inc & (diff < dtype(t) + dtype(2.0 * margin))).sum(1) for t in thresholds], 1)
    return inc.sum(1).astype(np.int64), kept.astype(np.int64)


def flips(top, selected=None):
    """{residue: [(atom a, atom b), ..]} of the residues whose type is in FLIPS and whose named atoms all exist (and are
    selected), by atom name."""
    out = {}
    for r, nm in enumerate(top.res_names):
        if nm not in FLIPS:
            continue
        first = int(top.first_atom[r])
        where = {a: first + k for k, a in enumerate(top.atom_names[r])}
        named = [tuple(pair.split("=")) for pair in FLIPS[nm].split()]
        if all(a in where and (selected is None or where[a] in selected) for pair in named for a in pair):
            out[r] = [(where[a], where[b]) for a, b in named]
    return out


def evaluate(model, ref, res, dtype=np.float64, sel=None, flip=None, **kw):
    """One structure against one frame -> dict.  sel: the atoms that take part, in this order; flip: {residue: [(a, b)]}
    (atom indices) of the symmetric residues, None: no symmetry.  A residue is exchanged iff the sum of `preserved` over its
    atoms and all thresholds is strictly greater with its own atoms exchanged and every other atom as it is."""
    model, ref, res = np.asarray(model), np.asarray(ref), np.asarray(res)
    n_res = int(res.max()) + 1
    sel = np.arange(res.shape[0]) if sel is None else np.asarray(sel)
    T = len(kw.get("thresholds", THRESHOLDS))
    out = dict(swapped=np.zeros(n_res, dtype=bool))
    atoms = np.concatenate([model[sel], ref[sel]])
    if not np.isfinite(atoms).all():
        out.update(finite=False, atom_total=np.full(sel.shape[0], -1), atom_preserved=np.full((sel.shape[0], T), -1),
                   residue_total=np.full(n_res, -1), residue_preserved=np.full((n_res, T), -1),
                   residue=np.full(n_res, np.nan), score=np.nan)
        out["global"] = np.nan
        return out
    chosen = np.array(model, copy=True)
    for r, pairs in (flip or {}).items():
        own = np.nonzero(res[sel] == r)[0]
        flipped = np.array(model, copy=True)
        for a, b in pairs:
            flipped[[a, b]] = model[[b, a]]
        # the rows of the residue read the exchanged coordinates; no partner of theirs lies in the residue
        keep = counts(model[sel], ref[sel], res[sel], dtype, rows=own, **kw)[1].sum()
        swap = counts(flipped[sel], ref[sel], res[sel], dtype, rows=own, **kw)[1].sum()
        if swap > keep:
            out["swapped"][r] = True
            chosen[res == r] = flipped[res == r]
    total, kept = counts(chosen[sel], ref[sel], res[sel], dtype, **kw)
    r_total, r_kept = np.zeros(n_res, dtype=np.int64), np.zeros((n_res, T), dtype=np.int64)
    np.add.at(r_total, res[sel], total)
    np.add.at(r_kept, res[sel], kept)
    out.update(finite=True, atom_total=total, atom_preserved=kept, residue_total=r_total, residue_preserved=r_kept,
               residue=scores(r_total, r_kept), score=scores(total.sum(), kept.sum(0)))
    out["global"] = out["score"]
    return out


def scores(total, kept):
    """sum_k kept / (T * total) in float64 from integers (one division), NaN where total is 0."""
    total, kept = np.asarray(total, dtype=np.int64), np.asarray(kept, dtype=np.int64)
    T = kept.shape[-1]
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(total > 0, kept.sum(-1).astype(np.float64) / (T * total).astype(np.float64), np.nan)


def sandwich(model, ref, res, **kw):
    """((total, preserved) lower, (total, preserved) upper, undecided share): float64 counts with the inclusion cut moved by
    -+ eps and every threshold by -+ 2 eps, eps = EPS_FACTOR * max |coordinate|; the share of the decisions between the two
    in (T + 1) * sum(total)."""
    eps = EPS_FACTOR * max(np.abs(np.asarray(model, dtype=np.float64)).max(), np.abs(np.asarray(ref, dtype=np.float64)).max())
    lo = counts(model, ref, res, np.float64, margin=-eps, **kw)
    hi = counts(model, ref, res, np.float64, margin=eps, **kw)
    mid = counts(model, ref, res, np.float64, **kw)
    between = (hi[0] - lo[0]).sum() + (hi[1] - lo[1]).sum()
    return lo, hi, between / ((mid[1].shape[1] + 1) * max(int(mid[0].sum()), 1))


# ------------------------------------------------------------------------------------------------------ the test inputs
_CHAINS = {}


def chain(n, seed=7):
    """(Topology, xyz float32 [n_atoms, 3]) of stereo_ref.planted(n, seed); built once."""
    if (n, seed) not in _CHAINS:
        top, xyz = sr.build_chain(**sr.planted(n, seed))
        _CHAINS[(n, seed)] = (top, np.ascontiguousarray(xyz, dtype=np.float32))
    return _CHAINS[(n, seed)]


def noisy(xyz, sigma, seed, copies=1):
    """float32 [copies, n_atoms, 3]: the frame plus seeded Gaussian noise, rounded to float32 before anything reads it."""
    rng = np.random.default_rng(seed)
    return (xyz.astype(np.float64)[None] + sigma * rng.standard_normal((copies,) + xyz.shape)).astype(np.float32)


def residues(top):
    return np.asarray(top.residue_of_atom)


def lattice(n, spacing=3.0):
    """float32 [n, 3]: n single-atom residues on a cubic lattice (exactly representable coordinates)."""
    side = int(np.ceil(n ** (1.0 / 3.0)))
    i = np.arange(n)
    return (np.stack([i % side, (i // side) % side, i // (side * side)], 1) * spacing).astype(np.float32)


def toy():
    """The hand-derived two-residue case: residue 0 is one atom at the origin, residue 1 five atoms at x = 1 .. 5; the model
    moves those by 0.25, 0.75, 1.5, 3 and 5 along x.  Every coordinate and every distance is exact in float32.
    -> (model, ref, res_ptr, the sum over k of each atom's preserved counts, the score)."""
    ref = np.zeros((6, 3), dtype=np.float32)
    ref[1:, 0] = [1, 2, 3, 4, 5]
    model = ref.copy()
    model[1:, 0] += np.array([0.25, 0.75, 1.5, 3.0, 5.0], dtype=np.float32)
    # atom 0 keeps 1, 2, 3, 4 of its five partners at 0.5, 1, 2, 4; the partners keep 4, 3, 2, 1, 0 thresholds of their one
    return model, ref, [0, 1, 6], [10, 4, 3, 2, 1, 0], 20.0 / 40.0
