"""Ground truth and float64 reference of the stereochemistry check (metrics.stereo_check, codlad_stereo_check).

`build_chain` places the atoms of a sequence by NeRF from GIVEN torsions and handedness, in the atom order of
`template_topology`, so the planted angles, inversions and peptide-bond classes are known without evaluating anything.
`reference` evaluates the nine columns, the flags and the counts from coordinates by atom NAME, with a table of its own
(CHI_X below, in the form the residue types are usually listed); it shares no code with `metrics.stereo_tables`.  The same
formula runs in float64 (the reference) and in float32 (numpy, one rounding per operation in the kernel's order): the
difference of the two on the same inputs is ref_dev, the deviation the device is allowed four times over.
"""
import numpy as np

from codlad_amd.utils.cg_input import template_topology

COLUMNS = ("phi", "psi", "omega", "chi1", "chi2", "chi3", "chi4", "v_ca", "v_side")
COUNTS = ("inverted_ca", "inverted_side", "cis_pro", "cis_nonpro", "twisted", "undefined")
INVERTED_CA, INVERTED_SIDE, CIS, TWISTED, UNDEFINED = 1, 2, 4, 8, 16

# chi_k = A-B-C-X per residue type: (A, B, C, X)
CHI_X = [
    {**{r: ("N", "CA", "CB", "CG") for r in "ARG ASN ASP GLN GLU HIS LEU LYS MET PHE PRO TRP TYR".split()},
     **{r: ("N", "CA", "CB", "CG1") for r in ("ILE", "VAL")}, **{r: ("N", "CA", "CB", "OG") for r in ("SER", "SEP")},
     **{r: ("N", "CA", "CB", "OG1") for r in ("THR", "TPO")}, "CYS": ("N", "CA", "CB", "SG")},
    {**{r: ("CA", "CB", "CG", "CD") for r in "ARG GLN GLU LYS PRO".split()},
     **{r: ("CA", "CB", "CG", "OD1") for r in ("ASN", "ASP")}, "HIS": ("CA", "CB", "CG", "ND1"),
     **{r: ("CA", "CB", "CG", "CD1") for r in "LEU PHE TRP TYR".split()}, "MET": ("CA", "CB", "CG", "SD"),
     "ILE": ("CA", "CB", "CG1", "CD1")},
    {"ARG": ("CB", "CG", "CD", "NE"), "GLN": ("CB", "CG", "CD", "OE1"), "GLU": ("CB", "CG", "CD", "OE1"),
     "LYS": ("CB", "CG", "CD", "CE"), "MET": ("CB", "CG", "SD", "CE")},
    {"ARG": ("CG", "CD", "NE", "CZ"), "LYS": ("CG", "CD", "CE", "NZ")},
]
SIDE_X = {"THR": "OG1", "TPO": "OG1", "ILE": "CG1"}
N_CHI = {r: sum(r in t for t in CHI_X) for r in
         "ALA ARG ASN ASP CYS GLN GLU GLY HIS ILE LEU LYS MET PHE PRO SER THR TRP TYR VAL TPO SEP".split()}

# ideal geometry (Engh & Huber): bond lengths in A, angles in degrees
D_N_CA, D_CA_C, D_C_N, D_C_O, D_CA_CB = 1.458, 1.525, 1.329, 1.231, 1.530
A_N_CA_C, A_CA_C_N, A_C_N_CA, A_CA_C_O, A_N_CA_CB = 111.0, 116.2, 121.7, 120.5, 110.5
T_CB_L = -122.5                    # torsion(C, N, CA, CB) of an L residue; a D residue has +122.5
D_SIDE, A_SIDE = 1.52, 111.0       # every side-chain bond and angle of the builder
T_BRANCH = -120.0                  # torsion(N, CA, CB, CG2) - chi1 of natural (2S,3R)-THR and (2S,3S)-ILE; flipped: +120


def place(a, b, c, bond, angle, torsion):
    """NeRF: the point d with |d - c| = bond, angle(b, c, d) = angle and torsion(a, b, c, d) = torsion (degrees, IUPAC)."""
    ang, tor = np.deg2rad(angle), np.deg2rad(torsion)
    bc = (c - b) / np.linalg.norm(c - b)
    n = np.cross(b - a, bc)
    n /= np.linalg.norm(n)
    m = np.cross(n, bc)
    d2 = np.array([-bond * np.cos(ang), bond * np.sin(ang) * np.cos(tor), bond * np.sin(ang) * np.sin(tor)])
    return c + d2[0] * bc + d2[1] * m + d2[2] * n


def build_chain(seq, phi, psi, omega, chi, d_ca=None, d_side=None, chain_breaks=()):
    """-> (Topology, xyz float64 [n_atoms, 3]).  seq: residue names; phi, psi, omega [n] and chi [n, 4] in degrees (omega[i]
    is the peptide bond INTO residue i; entries a residue does not have are ignored); d_ca [n] bool: the residue's CA is D;
    d_side [n] bool: the CB of a THR / TPO / ILE is inverted; chain_breaks: the residues that start a new chain.
    N, CA, C, O, CB and the atoms of the chi path are placed from these angles; the THR / ILE branch atom CG2 at chi1 -/+
    120; every other template atom off the last three placed ones (non-degenerate, read by no quantity)."""
    n = len(seq)
    d_ca = np.zeros(n, bool) if d_ca is None else np.asarray(d_ca, bool)
    d_side = np.zeros(n, bool) if d_side is None else np.asarray(d_side, bool)
    starts = {0} | set(int(b) for b in chain_breaks)
    chain, ids = -1, []
    for i in range(n):
        chain += i in starts
        ids.append(chain)
    top = template_topology(list(seq), chain_ids=ids)
    xyz = np.full((top.n_atoms, 3), np.nan)
    for i, nm in enumerate(seq):
        at = {a: top.atom(i, a) for a in top.atom_names[i]}
        if i in starts:                                   # a fresh frame, chains 40 A apart
            origin = np.array([0.0, 40.0 * ids[i], 0.0])
            N = origin
            CA = origin + np.array([D_N_CA, 0.0, 0.0])
            t = np.deg2rad(A_N_CA_C)
            C = CA + D_CA_C * np.array([-np.cos(t), np.sin(t), 0.0])
        else:
            pN, pCA, pC = (xyz[top.atom(i - 1, a)] for a in ("N", "CA", "C"))
            N = place(pN, pCA, pC, D_C_N, A_CA_C_N, psi[i - 1])
            CA = place(pCA, pC, N, D_N_CA, A_C_N_CA, omega[i])
            C = place(pC, N, CA, D_CA_C, A_N_CA_C, phi[i])
        xyz[at["N"]], xyz[at["CA"]], xyz[at["C"]] = N, CA, C
        xyz[at["O"]] = place(N, CA, C, D_C_O, A_CA_C_O, psi[i] + 180.0)
        placed = ["N", "CA", "C", "O"]
        if "CB" in at:
            xyz[at["CB"]] = place(C, N, CA, D_CA_CB, A_N_CA_CB, -T_CB_L if d_ca[i] else T_CB_L)
            placed.append("CB")
            path = ["N", "CA", "CB"]
            for k in range(N_CHI[nm]):
                a, b, c, x = CHI_X[k][nm]
                assert [a, b, c] == path[-3:]
                xyz[at[x]] = place(xyz[at[a]], xyz[at[b]], xyz[at[c]], D_SIDE, A_SIDE, chi[i][k])
                path.append(x)
                placed.append(x)
            if nm in SIDE_X:
                xyz[at["CG2"]] = place(N, CA, xyz[at["CB"]], D_SIDE, A_SIDE, chi[i][0] + (-T_BRANCH if d_side[i] else T_BRANCH))
                placed.append("CG2")
        for k, a in enumerate(top.atom_names[i]):
            if a not in placed:
                p, q, r = (xyz[at[b]] for b in placed[-3:])
                xyz[at[a]] = place(p, q, r, 1.4, 115.0, 60.0 + 37.0 * k)
                placed.append(a)
    assert np.isfinite(xyz).all()
    return top, xyz


def site_names(top):
    """[n_res][9]: the (residue, atom name) of the four atoms of each quantity, None where the residue has none."""
    out = []
    for i, nm in enumerate(top.res_names):
        prev = i > 0 and top.chain_ids[i - 1] == top.chain_ids[i]
        nxt = i + 1 < top.n_residues and top.chain_ids[i + 1] == top.chain_ids[i]
        here = lambda *names: [(i, a) for a in names]                                                        # noqa: E731
        row = [[(i - 1, "C")] + here("N", "CA", "C") if prev else None,
               here("N", "CA", "C") + [(i + 1, "N")] if nxt else None,
               [(i - 1, "CA"), (i - 1, "C")] + here("N", "CA") if prev else None]
        row += [here(*CHI_X[k][nm]) if nm in CHI_X[k] else None for k in range(4)]
        row.append(here("CA", "N", "C", "CB") if nm != "GLY" else None)
        row.append(here("CB", "CA", SIDE_X[nm], "CG2") if nm in SIDE_X else None)
        out.append(row)
    return out


def site_index(top):
    """int64 [n_res, 9, 4] atom indices by name, -1 rows where the quantity does not exist."""
    idx = np.full((top.n_residues, 9, 4), -1, dtype=np.int64)
    for i, row in enumerate(site_names(top)):
        for q, atoms in enumerate(row):
            if atoms is not None:
                idx[i, q] = [top.atom(r, a) for r, a in atoms]
                assert (idx[i, q] >= 0).all()
    return idx


def readers(top, atom):
    """The residues with a quantity that reads atom index `atom`."""
    idx = site_index(top)
    return sorted(set(np.nonzero((idx == atom).any(axis=(1, 2)))[0].tolist()))


def _sub(a, b):
    return a - b


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def torsion(p0, p1, p2, p3):
    """IUPAC torsion in degrees in (-180, 180], in the dtype of the inputs; NaN where atan2's arguments are both 0."""
    dt = p0.dtype.type
    with np.errstate(all="ignore"):
        b1, b2, b3 = _sub(p1, p0), _sub(p2, p1), _sub(p3, p2)
        n1, n2 = _cross(b1, b2), _cross(b2, b3)
        x = _dot(n1, n2)
        y = _dot(_cross(n1, n2), b2) / np.sqrt(_dot(b2, b2))
        deg = np.arctan2(y, x) * dt(180.0 / np.pi)
    deg = np.where((x == 0) & (y == 0), dt(np.nan), deg)
    return np.where(deg == -180.0, dt(180.0), deg)


def volume(p0, p1, p2, p3):
    with np.errstate(all="ignore"):
        return _dot(_sub(p1, p0), _cross(_sub(p2, p0), _sub(p3, p0)))


def bond_angles(xyz, top):
    """The two bond angles (degrees, float64) inside every existing torsion: [S, n_res, 7, 2], NaN where absent."""
    idx = site_index(top)[:, :7]
    x = np.asarray(xyz, dtype=np.float64).reshape(-1, top.n_atoms, 3)
    p = x[:, np.maximum(idx, 0)]
    out = []
    for k in (0, 1):
        u, v = p[..., k, :] - p[..., k + 1, :], p[..., k + 2, :] - p[..., k + 1, :]
        with np.errstate(invalid="ignore", divide="ignore"):          # absent rows read atom 0 four times
            c = (u * v).sum(-1) / np.sqrt((u * u).sum(-1) * (v * v).sum(-1))
        out.append(np.rad2deg(np.arccos(np.clip(c, -1, 1))))
    ang = np.stack(out, -1)
    ang[:, (idx < 0).any(-1)] = np.nan
    return ang


def reference(xyz, top, dtype=np.float64):
    """xyz [S, n_atoms, 3] (or [n_atoms, 3]) -> (values [S, n_res, 9] in `dtype`, flags uint8 [S, n_res], counts int32
    [S, 6]).  The arithmetic runs in `dtype` from the coordinates cast to it."""
    idx = site_index(top)
    exists = (idx >= 0).all(-1)                                               # [R, 9]
    x = np.asarray(xyz).reshape(-1, top.n_atoms, 3).astype(dtype)
    p = x[:, np.maximum(idx, 0)]                                              # [S, R, 9, 4, 3]
    p0, p1, p2, p3 = (p[..., k, :] for k in range(4))
    values = np.concatenate([torsion(p0[..., :7, :], p1[..., :7, :], p2[..., :7, :], p3[..., :7, :]),
                             volume(p0[..., 7:, :], p1[..., 7:, :], p2[..., 7:, :], p3[..., 7:, :])], -1).astype(dtype)
    values = np.where(exists[None], values, dtype(np.nan))
    fin = np.isfinite(values)
    with np.errstate(invalid="ignore"):
        w = np.abs(values[..., 2])
        flags = (INVERTED_CA * (fin[..., 7] & ~(values[..., 7] > 0)) + INVERTED_SIDE * (fin[..., 8] & ~(values[..., 8] > 0)) +
                 CIS * (w < 30.0) + TWISTED * ((w >= 30.0) & (w <= 150.0)) +
                 UNDEFINED * (exists[None] & ~fin).any(-1)).astype(np.uint8)
    pro = np.array([nm == "PRO" for nm in top.res_names])[None]
    cis = (flags & CIS) > 0
    counts = np.stack([((flags & INVERTED_CA) > 0).sum(1), ((flags & INVERTED_SIDE) > 0).sum(1), (cis & pro).sum(1),
                       (cis & ~pro).sum(1), ((flags & TWISTED) > 0).sum(1), ((flags & UNDEFINED) > 0).sum(1)], 1)
    return values, flags, counts.astype(np.int32)


def angle_diff(a, b):
    """|a - b| modulo 360 degrees, float64."""
    d = np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)) % 360.0
    return np.minimum(d, 360.0 - d)


# ------------------------------------------------------------------------------------------------------ the test inputs
RES22 = "ALA ARG ASN ASP CYS GLN GLU GLY HIS ILE LEU LYS MET PHE PRO SER THR TRP TYR VAL TPO SEP".split()
SIZES = (1, 2, 3, 63, 64, 65, 255, 256, 257, 600)
SHIFT = 1000.0


def planted(n, seed, chain_breaks=(), first=0):
    """Random inputs of build_chain for n residues cycling through the 22 templates from number `first` -> dict.  omega: trans 180 +/- 25,
    cis +/- 25 (about 10 %, PRO or not), twisted 35 .. 145 (about 5 %, either sign); about 10 % D residues and about 10 %
    flipped THR / TPO / ILE centres."""
    rng = np.random.default_rng(seed)
    seq = [RES22[(i + first) % 22] for i in range(n)]
    u = rng.random(n)
    mag = np.where(u < 0.10, rng.uniform(0, 25, n), np.where(u < 0.15, rng.uniform(35, 145, n), rng.uniform(155, 180, n)))
    omega = mag * rng.choice([-1.0, 1.0], n)
    omega[omega == -180.0] = 180.0
    return dict(seq=seq, phi=rng.uniform(-180, 180, n), psi=rng.uniform(-180, 180, n), omega=omega,
                chi=rng.uniform(-180, 180, (n, 4)), d_ca=rng.random(n) < 0.10, d_side=rng.random(n) < 0.10,
                chain_breaks=tuple(chain_breaks))


def planted_truth(top, pl):
    """What build_chain planted, in the reference's terms: (values float64 [n_res, 7] of the torsions that exist, NaN
    elsewhere; flags uint8 [n_res])."""
    idx = site_index(top)
    exists = (idx >= 0).all(-1)
    n = top.n_residues
    tors = np.concatenate([np.stack([pl["phi"], pl["psi"], pl["omega"]], 1), pl["chi"]], 1)
    tors = np.where(exists[:, :7], tors, np.nan)
    w = np.abs(tors[:, 2])
    with np.errstate(invalid="ignore"):
        flags = (INVERTED_CA * (exists[:, 7] & pl["d_ca"]) + INVERTED_SIDE * (exists[:, 8] & pl["d_side"]) +
                 CIS * (w < 30.0) + TWISTED * ((w >= 30.0) & (w <= 150.0))).astype(np.uint8)
    assert flags.shape == (n,)
    return tors, flags
