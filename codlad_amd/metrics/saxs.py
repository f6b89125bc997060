"""Small-angle X-ray scattering profiles of an ensemble (codlad_saxs_debye, csrc/saxs_kernels.hip): the Debye sum over all
atom pairs of every structure, with united-atom form factors (a heavy atom and the hydrogens riding on it) in a displaced
solvent; and the hydration model on top of it (codlad_saxs_partials, codlad_saxs_hydration_fit,
csrc/saxs_hydration_kernels.hip): six partial Debye sums from one pass over the pairs, from which the profile at any
excluded-volume scale c1 and hydration-shell weight c2 is a float64 combination, and the fit of both to a curve.  No
interpolation between q grids."""
import numpy as np
import torch

from .. import _lib
from . import _inputs

SAXS_MAX_Q, SAXS_MAX_TYPES, SAXS_Q_CHUNK = _lib.SAXS_MAX_Q, _lib.SAXS_MAX_TYPES, _lib.SAXS_Q_CHUNK
SAXS_X_MAX, SAXS_X_SMALL = _lib.SAXS_X_MAX, _lib.SAXS_X_SMALL
SAXS_MAX_EXTENT = 2000.0           # A: the largest distance q * r is held below X_MAX for (q <= X_MAX / SAXS_MAX_EXTENT)
SAXS_Q_LIMIT = SAXS_X_MAX / SAXS_MAX_EXTENT

# Cromer-Mann: f(q) = sum_4 a_i exp(-b_i (q / 4 pi)^2) + c (International Tables for Crystallography, vol. C); a, b, c
CROMER_MANN = {
    "H": ((0.489918, 0.262003, 0.196767, 0.049879), (20.6593, 7.74039, 49.5519, 2.20159), 0.001305),
    "C": ((2.3100, 1.0200, 1.5886, 0.8650), (20.8439, 10.2075, 0.5687, 51.6512), 0.2156),
    "N": ((12.2126, 3.1322, 2.0125, 1.1663), (0.0057, 9.8933, 28.9975, 0.5826), -11.529),
    "O": ((3.0485, 2.2868, 1.5463, 0.8670), (13.2771, 5.7011, 0.3239, 32.9089), 0.2508),
    "P": ((6.4345, 4.1791, 1.7800, 1.4908), (1.9067, 27.1570, 0.5260, 68.1645), 1.1149),
    "S": ((6.9053, 5.2034, 1.4379, 1.5863), (1.4679, 22.2151, 0.2536, 56.1720), 0.8669),
}
ATOMIC_VOLUME = {"H": 5.15, "C": 16.44, "N": 2.49, "O": 9.13, "P": 5.73, "S": 19.86}       # A^3 (Fraser et al. 1978)

# hydrogens riding on the side-chain heavy atoms at neutral pH; the backbone is _backbone_h's
_SIDE_H = {
    "ALA": {"CB": 3}, "GLY": {},
    "ARG": {"CB": 2, "CG": 2, "CD": 2, "NE": 1, "CZ": 0, "NH1": 2, "NH2": 2},
    "ASP": {"CB": 2, "CG": 0, "OD1": 0, "OD2": 0}, "ASN": {"CB": 2, "CG": 0, "OD1": 0, "ND2": 2},
    "CYS": {"CB": 2, "SG": 1}, "GLU": {"CB": 2, "CG": 2, "CD": 0, "OE1": 0, "OE2": 0},
    "GLN": {"CB": 2, "CG": 2, "CD": 0, "OE1": 0, "NE2": 2},
    "HIS": {"CB": 2, "CG": 0, "ND1": 0, "CD2": 1, "CE1": 1, "NE2": 1},
    "HID": {"CB": 2, "CG": 0, "ND1": 1, "CD2": 1, "CE1": 1, "NE2": 0},
    "ILE": {"CB": 1, "CG1": 2, "CG2": 3, "CD1": 3}, "LEU": {"CB": 2, "CG": 1, "CD1": 3, "CD2": 3},
    "LYS": {"CB": 2, "CG": 2, "CD": 2, "CE": 2, "NZ": 3}, "MET": {"CB": 2, "CG": 2, "SD": 0, "CE": 3},
    "PHE": {"CB": 2, "CG": 0, "CD1": 1, "CD2": 1, "CE1": 1, "CE2": 1, "CZ": 1},
    "PRO": {"CB": 2, "CG": 2, "CD": 2}, "SER": {"CB": 2, "OG": 1}, "THR": {"CB": 1, "OG1": 1, "CG2": 3},
    "TRP": {"CB": 2, "CG": 0, "CD1": 1, "CD2": 0, "NE1": 1, "CE2": 0, "CE3": 1, "CZ2": 1, "CZ3": 1, "CH2": 1},
    "TYR": {"CB": 2, "CG": 0, "CD1": 1, "CD2": 1, "CE1": 1, "CE2": 1, "CZ": 0, "OH": 1},
    "VAL": {"CB": 1, "CG1": 3, "CG2": 3},
    "SEP": {"CB": 2, "OG": 0, "P": 0, "OE1": 0, "OE2": 0, "OE3": 0},
    "TPO": {"CB": 1, "OG1": 0, "CG2": 3, "P": 0, "OE1": 0, "OE2": 0, "OE3": 0},
}


def _backbone_h(res, name, chain_start):
    if name == "N":
        return (0 if res == "PRO" else 1) + (2 if chain_start else 0)
    if name == "CA":
        return 2 if res == "GLY" else 1
    return 0 if name in ("C", "O", "OXT") else None


def implicit_hydrogens(top):
    """int64 numpy [n_atoms]: the hydrogens riding on each heavy atom of the topology at neutral pH, by residue and atom
    name (the 20 standard residues, HID, SEP, TPO).  The N of a chain's first residue carries two more (the terminal
    NH3+).  A residue or an atom name the table does not know raises ValueError naming it."""
    out = np.zeros(top.n_atoms, dtype=np.int64)
    for r, (res, names) in enumerate(zip(top.res_names, top.atom_names)):
        if res not in _SIDE_H:
            raise ValueError(f"implicit_hydrogens: no hydrogen table for residue {res} (known: {' '.join(sorted(_SIDE_H))})")
        start = r == 0 or top.chain_ids[r] != top.chain_ids[r - 1]
        for a, name in enumerate(names):
            h = _backbone_h(res, name, start)
            if h is None:
                h = _SIDE_H[res].get(name)
            if h is None:
                raise ValueError(f"implicit_hydrogens: residue {res} has no atom named {name} in the hydrogen table")
            out[int(top.first_atom[r]) + a] = h
    return out


def _cromer_mann(element, s2, table):
    a, b, c = table[element]
    return sum(ai * np.exp(-bi * s2) for ai, bi in zip(a, b)) + c


def form_factors(q, groups, solvent_density=0.334, cromer_mann=None, volumes=None):
    """float64 numpy [len(groups), Q]: the form factor of every group (element, n_H) - a heavy atom with n_H hydrogens
    riding on it - at the momentum transfers q (1/A): the vacuum factor f_el(q) + n_H f_H(q) (CROMER_MANN, or the dict
    given) minus the displaced solvent solvent_density * V * exp(-q^2 V^(2/3) / (4 pi)) (Fraser et al. 1978), V the sum of
    the group's ATOMIC_VOLUME (or the dict given).  solvent_density = 0: in vacuo.  An element not in a table raises
    ValueError."""
    cm = CROMER_MANN if cromer_mann is None else cromer_mann
    vol = ATOMIC_VOLUME if volumes is None else volumes
    q = np.asarray(q, dtype=np.float64).reshape(-1)
    groups = [(str(e).strip().upper(), int(h)) for e, h in groups]
    unknown = sorted({e for e, _h in groups} - (set(cm) & set(vol)))
    if unknown or (any(h for _e, h in groups) and not ("H" in cm and "H" in vol)):
        raise ValueError(f"no form factor for element(s) {unknown or ['H']} (known: {', '.join(sorted(set(cm) & set(vol)))})")
    if any(h < 0 for _e, h in groups) or not float(solvent_density) >= 0:
        raise ValueError("form_factors: hydrogen counts and the solvent density must be non-negative")
    s2 = (q / (4.0 * np.pi)) ** 2
    out = np.empty((len(groups), q.shape[0]), dtype=np.float64)
    for g, (e, h) in enumerate(groups):
        vac = _cromer_mann(e, s2, cm) + (h * _cromer_mann("H", s2, cm) if h else 0.0)
        v = vol[e] + (h * vol["H"] if h else 0.0)
        out[g] = vac - float(solvent_density) * v * np.exp(-q * q * v ** (2.0 / 3.0) / (4.0 * np.pi))
    return out


def _host(a, dtype):
    return np.ascontiguousarray(a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a), dtype=dtype)


def _saxs_tables(types, table, q, dev):
    """The checked tables of codlad_saxs_debye on `dev`: (type int32 [n], ff float32 [T, Q], q float32 [Q])."""
    q64 = _host(q, np.float64).reshape(-1)
    tab = _host(table, np.float64)
    typ = _host(types, np.int64).reshape(-1)
    if tab.ndim != 2 or tab.shape[1] != q64.shape[0] or not q64.shape[0]:
        raise ValueError(f"saxs: the table must be [T, Q] with Q = len(q) >= 1, got {tab.shape} for {q64.shape[0]} q values")
    if q64.shape[0] > SAXS_MAX_Q or not 1 <= tab.shape[0] <= SAXS_MAX_TYPES:
        raise ValueError(f"saxs: at most {SAXS_MAX_Q} q values and 1 .. {SAXS_MAX_TYPES} atom types, got {q64.shape[0]} and {tab.shape[0]}")
    if not (np.isfinite(q64).all() and (q64 >= 0).all() and (q64 <= SAXS_Q_LIMIT).all()):
        raise ValueError(f"saxs: every q must be a number in [0, {SAXS_Q_LIMIT}] 1/A (q * r stays below {SAXS_X_MAX} for "
                         f"distances up to {SAXS_MAX_EXTENT} A)")
    with np.errstate(over="ignore"):
        tab32 = tab.astype(np.float32)
    if not np.isfinite(tab32).all():
        raise ValueError("saxs: a form-factor table entry is not a finite float32 number")
    if not typ.shape[0] or typ.min() < 0 or typ.max() >= tab.shape[0]:
        raise ValueError(f"saxs: every atom type must be in [0, {tab.shape[0]})")
    return (torch.from_numpy(typ.astype(np.int32)).to(dev), torch.from_numpy(tab32).to(dev),
            torch.from_numpy(q64.astype(np.float32)).to(dev))


def _saxs_launch(xyz, typ, ff, q, with_mean=False):
    x = _inputs.structures(xyz, "saxs: xyz", typ.shape[0])
    dev = x.device
    S, n, Q = x.shape[0], x.shape[1], q.shape[0]
    n_wg = ((n + 63) // 64 + 1) // 2
    partial = torch.empty(S, n_wg, Q, dtype=torch.float64, device=dev)
    I = torch.empty(S, Q, dtype=torch.float64, device=dev)
    mean = torch.empty(Q, dtype=torch.float64, device=dev) if with_mean else None
    finite = torch.empty(S, dtype=torch.uint8, device=dev)
    p = _lib.ptr
    rc = _lib.lib().codlad_saxs_debye(p(x), S, n, p(typ), ff.shape[0], p(ff), p(q), Q, p(partial), p(I), p(mean), p(finite),
                                      _lib.stream_ptr(dev))
    _lib.check(rc, "codlad_saxs_debye")
    out = dict(I=I, finite=finite.to(torch.bool))
    if with_mean:
        out["mean"] = mean
    return out


def saxs_profile_lists(xyz, types, table, q):
    """The raw Debye sum: xyz [S, n_atoms, 3] (device), types int [n_atoms] in [0, T), table [T, Q] (the form factor of
    every type at every q; rounded to float32) and q [Q] (1/A) -> dict: I float64 [S, Q] (device), finite bool [S].
    ValueError for a type outside the table, a q that is not a number in [0, SAXS_Q_LIMIT], a table entry that is not
    finite, or more than SAXS_MAX_Q q values / SAXS_MAX_TYPES types.  The tables are rebuilt on every call: for repeated
    calls on a protein use saxs_profile."""
    _inputs.need_cuda(xyz, "saxs: xyz")
    return _saxs_launch(xyz, *_saxs_tables(types, table, q, xyz.device))


def saxs_groups(top):
    """(groups, types): the distinct (element, n_H) of the topology's atoms, sorted, and int64 [n_atoms] into them."""
    pairs = list(zip((str(e).upper() for e in top.element), implicit_hydrogens(top).tolist()))
    groups = sorted(set(pairs))
    index = {g: k for k, g in enumerate(groups)}
    return groups, np.array([index[g] for g in pairs], dtype=np.int64)


def default_q():
    return np.linspace(0.0, 0.5, 51)


def saxs_profile(xyz, top, q=None, solvent_density=0.334):
    """SAXS profiles of xyz [S, n_atoms, 3] (device), S structures of the topology `top` -> dict of device tensors:
      q float32 [Q]        the momentum transfers as the kernel reads them (default: 51 points on [0, 0.5] 1/A)
      I float64 [S, Q]     the Debye sum of every structure with form_factors of saxs_groups(top)
      mean float64 [Q]     the average over the finite structures, added in index order; NaN if there is none
      finite bool [S]      False: a coordinate of the structure is NaN or +-inf - its row of I is NaN
      n_finite int         (a device tensor, int64 scalar)
    The groups and tables are built once per (topology, q, solvent_density, device).  No host transfer; sums in one order,
    so the bits repeat from call to call and a structure's row does not depend on the others of the call."""
    _inputs.need_cuda(xyz, "saxs: xyz")
    q64 = _host(default_q() if q is None else q, np.float64).reshape(-1)

    def build():
        groups, types = saxs_groups(top)
        return _saxs_tables(types, form_factors(q64, groups, solvent_density), q64, xyz.device)
    tables = _inputs.cached(top, "_saxs_tables", (q64.tobytes(), float(solvent_density), str(xyz.device)), build)
    out = _saxs_launch(xyz, *tables, with_mean=True)
    return dict(q=tables[2], I=out["I"], mean=out["mean"], finite=out["finite"], n_finite=out["finite"].sum())


def saxs_fit(I_calc, q, I_exp, sigma):
    """The scale and the reduced chi^2 of a computed curve against an experiment on the SAME q grid (pass the
    experiment's grid as `q` of saxs_profile: there is no interpolation).  float64 on the device of I_calc:
    c = sum(I_exp I_calc / sigma^2) / sum(I_calc^2 / sigma^2), chi2 = sum(((c I_calc - I_exp) / sigma)^2) / (Q - 1).
    -> dict(scale, chi2), scalar tensors."""
    _inputs.need_cuda(I_calc, "saxs_fit: I_calc")
    dev = I_calc.device
    calc = I_calc.detach().to(torch.float64).reshape(-1)
    exp, sig, qq = (torch.as_tensor(t).detach().to(device=dev, dtype=torch.float64).reshape(-1) for t in (I_exp, sigma, q))
    if not (calc.shape == exp.shape == sig.shape == qq.shape) or calc.shape[0] < 2:
        raise ValueError("saxs_fit: I_calc, q, I_exp and sigma must be four curves of the same length >= 2")
    if not bool((sig > 0).all()):
        raise ValueError("saxs_fit: every sigma must be positive")
    w = 1.0 / (sig * sig)
    scale = (exp * calc * w).sum() / (calc * calc * w).sum()
    chi2 = (((scale * calc - exp) / sig) ** 2).sum() / float(calc.shape[0] - 1)
    return dict(scale=scale, chi2=chi2)


# ---------------------------------------------------------------------------------- hydration shell and fitted contrast --
SAXS_HYD_PARTIALS, SAXS_HYD_Q_CHUNK, SAXS_HYD_MAX_GRID = _lib.SAXS_HYD_PARTIALS, _lib.SAXS_HYD_Q_CHUNK, _lib.SAXS_HYD_MAX_GRID
SAXS_PARTIAL_NAMES = ("tt", "td", "dd", "ts", "ds", "ss")
SAXS_R_M = 1.62                    # A: the mean atomic radius of the expansion factor (CRYSOL, FoXS)


def default_c1():
    """FoXS's range of the excluded-volume scale: 0.95 .. 1.05 in steps of 0.005."""
    return np.arange(21, dtype=np.float64) * 0.005 + 0.95


def default_c2():
    """FoXS's range of the hydration-shell weight: -2.0 .. 4.0 in steps of 0.1."""
    return np.arange(61, dtype=np.float64) * 0.1 - 2.0


def expansion_factor(q, c1, r_m=SAXS_R_M):
    """float64 numpy [len(c1), Q]: G(q, c1) = c1^3 exp(-(4 pi / 3)^(3/2) q^2 r_m^2 (c1^2 - 1) / (4 pi)), the scale of the
    displaced-solvent term when every atomic volume grows by c1^3 (CRYSOL / FoXS); G(q, 1) = 1 exactly."""
    q = np.asarray(q, dtype=np.float64).reshape(1, -1)
    c1 = np.asarray(c1, dtype=np.float64).reshape(-1, 1)
    return c1 ** 3 * np.exp(-((4.0 * np.pi / 3.0) ** 1.5 * q * q * float(r_m) ** 2 * (c1 * c1 - 1.0)) / (4.0 * np.pi))


def _partials_launch(xyz, typ, ff_t, ff_d, weight, q, with_mean=False):
    x = _inputs.structures(xyz, "saxs: xyz", typ.shape[0])
    dev = x.device
    S, n, Q = x.shape[0], x.shape[1], q.shape[0]
    _inputs.need_cuda(weight, "saxs: weight")
    if tuple(weight.shape) != (S, n):
        raise ValueError(f"saxs: weight must be [S, n_atoms] = {(S, n)}, one number per atom of every structure, got {tuple(weight.shape)}")
    wt = weight.detach().to(torch.float32).contiguous()
    n_wg = ((n + 63) // 64 + 1) // 2
    partial = torch.empty(S, n_wg, SAXS_HYD_PARTIALS, Q, dtype=torch.float64, device=dev)
    P = torch.empty(S, SAXS_HYD_PARTIALS, Q, dtype=torch.float64, device=dev)
    mean = torch.empty(SAXS_HYD_PARTIALS, Q, dtype=torch.float64, device=dev) if with_mean else None
    finite = torch.empty(S, dtype=torch.uint8, device=dev)
    p = _lib.ptr
    rc = _lib.lib().codlad_saxs_partials(p(x), S, n, p(typ), ff_t.shape[0], p(ff_t), p(ff_d), p(wt), p(q), Q, p(partial), p(P),
                                         p(mean), p(finite), _lib.stream_ptr(dev))
    _lib.check(rc, "codlad_saxs_partials")
    out = dict(P=P, finite=finite.to(torch.bool))
    if with_mean:
        out["mean"] = mean
    return out


def saxs_partials_lists(xyz, types, table_t, table_d, weight, q):
    """The six partial Debye sums of the hydration model: xyz [S, n_atoms, 3] (device), types int [n_atoms] in [0, T),
    table_t and table_d [T, Q] (in-solvent form factor and displaced solvent of every type; rounded to float32), weight
    [S, n_atoms] (device; the exposed fraction s_i of every atom of every structure) and q [Q] -> dict: P float64
    [S, 6, Q] (device) in the order SAXS_PARTIAL_NAMES, P_ab = sum_i a_i b_i + sum_{i<j} (a_i b_j + b_i a_j) sinc(q r_ij);
    finite bool [S], False where a coordinate or a weight is NaN or +-inf (six rows of NaN).  P[:, 0] has the bits of
    saxs_profile_lists(xyz, types, table_t, q)["I"].  The refusals of saxs_profile_lists, for both tables."""
    _inputs.need_cuda(xyz, "saxs: xyz")
    typ, ff_t, qd = _saxs_tables(types, table_t, q, xyz.device)
    _typ, ff_d, _q = _saxs_tables(types, table_d, q, xyz.device)
    return _partials_launch(xyz, typ, ff_t, ff_d, weight, qd)


def saxs_partials(xyz, top, q=None, solvent_density=0.334, probe=1.4, n_points=960):
    """The partial profiles of xyz [S, n_atoms, 3] (device), S structures of the topology `top`, from which saxs_combine
    and saxs_hydration_fit make I(q; c1, c2) -> dict of device tensors:
      q float32 [Q]              as saxs_profile
      P float64 [S, 6, Q]        tt, td, dd, ts, ds, ss of t = form_factors(q, groups, solvent_density), d = form_factors(q,
                                 groups, 0) - t and s = exposure; P[:, 0] has the bits of saxs_profile's I
      mean float64 [6, Q]        the average over the finite structures, added in index order; NaN if there is none
      finite bool [S], n_finite  as saxs_profile
      exposure float32 [S, n]    sasa(xyz, top, probe, n_points)["exposed"] / n_points: the share of an atom's test points
                                 that no other atom's sphere contains (computed on the device, no host transfer)
      water float64 [Q]          form_factors(q, [("O", 2)], solvent_density): the form factor of a shell water
    The tables are built once per (topology, q, solvent_density, device)."""
    from .observables import sasa
    _inputs.need_cuda(xyz, "saxs: xyz")
    q64 = _host(default_q() if q is None else q, np.float64).reshape(-1)

    def build():
        groups, types = saxs_groups(top)
        t = form_factors(q64, groups, solvent_density)
        typ, ff_t, qd = _saxs_tables(types, t, q64, xyz.device)
        _typ, ff_d, _q = _saxs_tables(types, form_factors(q64, groups, 0.0) - t, q64, xyz.device)
        water = torch.from_numpy(form_factors(q64, [("O", 2)], solvent_density)[0].copy()).to(xyz.device)
        return typ, ff_t, ff_d, qd, water
    typ, ff_t, ff_d, qd, water = _inputs.cached(top, "_saxs_hydration_tables",
                                                (q64.tobytes(), float(solvent_density), str(xyz.device)), build)
    exposure = sasa(xyz, top, probe=probe, n_points=n_points)["exposed"] / n_points
    out = _partials_launch(xyz, typ, ff_t, ff_d, exposure, qd, with_mean=True)
    return dict(q=qd, P=out["P"], mean=out["mean"], finite=out["finite"], n_finite=out["finite"].sum(), exposure=exposure,
                water=water)


def _hydration_tables(what, shape, q, water, c1, c2, r_m):
    """The host side of codlad_saxs_hydration_fit's arguments, checked: P's shape [..., 6, Q], q and water [Q], the grids
    -> float64 numpy (f_w [Q], G [len(c1), Q], c1, c2)."""
    if len(shape) < 2 or shape[-2] != SAXS_HYD_PARTIALS or shape[-1] < 1 or 0 in shape:
        raise ValueError(f"{what}: P must be [..., {SAXS_HYD_PARTIALS}, Q] (the partial profiles of saxs_partials), got {tuple(shape)}")
    Q = shape[-1]
    q64 = _host(q, np.float64).reshape(-1)
    fw = _host(water, np.float64).reshape(-1)
    if q64.shape[0] != Q or fw.shape[0] != Q or Q > SAXS_MAX_Q:
        raise ValueError(f"{what}: q and water must have the Q = {Q} <= {SAXS_MAX_Q} values of P, got {q64.shape[0]} and {fw.shape[0]}")
    if not (np.isfinite(q64).all() and (q64 >= 0).all() and (q64 <= SAXS_Q_LIMIT).all()):
        raise ValueError(f"{what}: every q must be a number in [0, {SAXS_Q_LIMIT}] 1/A")
    g1, g2 = _host(c1, np.float64).reshape(-1), _host(c2, np.float64).reshape(-1)
    if not g1.shape[0] or not g2.shape[0] or g1.shape[0] * g2.shape[0] > SAXS_HYD_MAX_GRID:
        raise ValueError(f"{what}: the grid of c1 and c2 must have 1 .. {SAXS_HYD_MAX_GRID} points, got {g1.shape[0]} x {g2.shape[0]}")
    if not (np.isfinite(g1).all() and (g1 > 0).all() and np.isfinite(g2).all() and np.isfinite(float(r_m)) and float(r_m) >= 0):
        raise ValueError(f"{what}: every c1 must be positive, every c2 a number and r_m non-negative")
    return fw, expansion_factor(q64, g1, r_m), g1, g2


def _fit_curves(Q, I_exp, sigma):
    """I_exp and sigma of saxs_hydration_fit, checked -> float64 numpy [Q] each."""
    exp, sig = _host(I_exp, np.float64).reshape(-1), _host(sigma, np.float64).reshape(-1)
    if exp.shape[0] != Q or sig.shape[0] != Q or Q < 2:
        raise ValueError(f"saxs_hydration_fit: I_exp and sigma must have the Q = {Q} >= 2 values of P, got {exp.shape[0]} and {sig.shape[0]}")
    if not (sig > 0).all():
        raise ValueError("saxs_hydration_fit: every sigma must be positive")
    return exp, sig


def _hydration_inputs(what, P, q, water, c1, c2, r_m):
    """-> (P [B, 6, Q] float64, the shape of P before the 6-axis, f_w, G, c2 on the device of P, and the grids as numpy)."""
    _inputs.need_cuda(P, f"{what}: P")
    fw, G, g1, g2 = _hydration_tables(what, tuple(P.shape), q, water, c1, c2, r_m)
    dev = P.device
    up = lambda a: torch.from_numpy(np.array(a, dtype=np.float64)).to(dev)     # noqa: E731 (a copy: the caller's may be read-only)
    Pb = P.detach().to(torch.float64).reshape(-1, SAXS_HYD_PARTIALS, P.shape[-1]).contiguous()
    return Pb, tuple(P.shape[:-2]), up(fw), up(G), up(g2), g1, g2


def saxs_combine(P, q, water, c1=1.0, c2=0.0, r_m=SAXS_R_M):
    """I(q; c1, c2) of partial profiles P [..., 6, Q] (device; saxs_partials' P or mean) -> float64 [..., Q]:
      I = P_tt + 2 (1 - G) P_td + (1 - G)^2 P_dd + 2 c2 f_w P_ts + 2 c2 f_w (1 - G) P_ds + c2^2 f_w^2 P_ss
    with G = expansion_factor(q, c1, r_m) and f_w = water, in float64 in the order include/codlad_hip.h states.  c1 scales
    the excluded volume (c1 = 1: as saxs_profile), c2 weighs the bound water on the exposed atoms.  (1, 0) returns P_tt."""
    Pb, lead, fw, G, g2, _g1, _g2 = _hydration_inputs("saxs_combine", P, q, water, [float(c1)], [float(c2)], r_m)
    I = torch.empty(Pb.shape[0], 1, Pb.shape[2], dtype=torch.float64, device=Pb.device)
    p = _lib.ptr
    rc = _lib.lib().codlad_saxs_hydration_fit(p(Pb), Pb.shape[0], Pb.shape[2], p(fw), p(G), 1, p(g2), 1, None, None, p(I), None,
                                              None, None, None, _lib.stream_ptr(Pb.device))
    _lib.check(rc, "codlad_saxs_hydration_fit")
    return I.reshape(*lead, Pb.shape[2])


def saxs_hydration_fit(P, q, water, I_exp, sigma, c1=None, c2=None, r_m=SAXS_R_M):
    """The (c1, c2) of a grid at which partial profiles P [6, Q] or [B, 6, Q] (device) fit an experiment on the SAME q
    grid best: for every grid point the scale and the reduced chi^2 of saxs_fit (sums over q ascending), then the smallest
    chi^2 - the lowest flat index i1 * len(c2) + i2 of a tie; a chi^2 that is not finite never wins.  c1, c2: the grids
    (default default_c1() x default_c2(), FoXS's ranges; at most SAXS_HYD_MAX_GRID points) -> dict of device tensors, with a
    leading [B] for a batch:
      c1, c2, scale, chi2 float64   at the best point (NaN when no chi^2 is finite)
      index int32                   its flat index, -1 when there is none
      I float64 [Q]                 the profile there (unscaled)
      chi2_grid, scale_grid float64 [len(c1), len(c2)]
    For an ensemble pass saxs_partials' mean: the fit is of the ensemble, not of a structure."""
    Pb, lead, fw, G, g2d, g1, g2 = _hydration_inputs("saxs_hydration_fit", P, q, water, default_c1() if c1 is None else c1,
                                                     default_c2() if c2 is None else c2, r_m)
    if len(lead) > 1:
        raise ValueError(f"saxs_hydration_fit: P must be [6, Q] or [B, 6, Q], got {tuple(P.shape)}")
    B, Q, n1, n2 = Pb.shape[0], Pb.shape[2], g1.shape[0], g2.shape[0]
    exp, sig = _fit_curves(Q, I_exp, sigma)
    dev = Pb.device
    exp_d, sig_d = torch.from_numpy(exp.copy()).to(dev), torch.from_numpy(sig.copy()).to(dev)
    scale = torch.empty(B, n1 * n2, dtype=torch.float64, device=dev)
    chi2 = torch.empty(B, n1 * n2, dtype=torch.float64, device=dev)
    best = torch.empty(B, dtype=torch.int32, device=dev)
    I = torch.empty(B, Q, dtype=torch.float64, device=dev)
    p = _lib.ptr
    rc = _lib.lib().codlad_saxs_hydration_fit(p(Pb), B, Q, p(fw), p(G), n1, p(g2d), n2, p(exp_d), p(sig_d), None, p(scale), p(chi2),
                                              p(best), p(I), _lib.stream_ptr(dev))
    _lib.check(rc, "codlad_saxs_hydration_fit")
    at = best.to(torch.int64).clamp(min=0)
    none = best < 0
    nan = torch.full((), float("nan"), dtype=torch.float64, device=dev)
    pick = lambda t: torch.where(none, nan, t)                                                      # noqa: E731
    out = dict(c1=pick(torch.from_numpy(g1.copy()).to(dev)[at // n2]), c2=pick(g2d[at % n2]),
               scale=pick(scale.gather(1, at[:, None])[:, 0]), chi2=pick(chi2.gather(1, at[:, None])[:, 0]), I=I, index=best,
               chi2_grid=chi2.reshape(B, n1, n2), scale_grid=scale.reshape(B, n1, n2))
    return out if lead else {k: v[0] for k, v in out.items()}
