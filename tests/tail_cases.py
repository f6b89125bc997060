"""Cases and rules of the decoder tail's float64 parity test (tests/test_tail_fp64_parity.py, GPU) and of the CPU test that
holds them to what they claim (tests/test_tail_cases_host.py): ic -> xyz per atom, xyz -> ic per quad, and the decision
kernels (VQ lookup, CG graph, bond graph, clash counts) by their float64 margin.  Nothing here touches a GPU.

1. ic -> xyz.  s[atom] is the smallest |a x b| / (|a| |b|) over the atom's own placement and the placements of every atom
   it was built from (the sine between the two reference directions of oracle/vae_decode.py::_place, in float64, carried
   along `orders`; a CA has s = 1).  err = the Euclidean distance to the float64 coordinates.  One bound for every atom:

       err_hip[atom] x s[atom] <= C x max(E_ref, FLOOR_ULP x max|x64|)

   E_ref = the fp32 oracle's largest err x s on the same inputs, C = 4.

2. xyz -> ic.  Per quad (A1, A2, A3, A4), with max|x| the largest coordinate of the quad's own four atoms and
   u = 2^-23 max|x| / min(|A1 - A2|, |A3 - A2|, |A4 - A3|): distance within C 2^-23 max|x|, bond angle within
   C max(u, 2^-23), dihedral within C max(u, 2^-23) / min(sin(A1, A2, A3), sin(A2, A3, A4)); angles modulo 2 pi.

3. Decisions.  The decision and its margin in float64 from the device's own inputs; where the margin exceeds the stated
   rounding bound the device must equal float64, below it the fp32 oracle.  Planted ties are exact by construction.
"""
import functools

import numpy as np
import torch

from codlad_amd import metrics as gm
from codlad_amd import synth
from codlad_amd.utils import dataset_builder as db
from oracle import ic_build
from oracle import metrics as om
from oracle import vae_decode as odec
from tests import cases

C = 4.0
FLOOR_ULP = 2.0 ** -23
S_MIN = 1e-3                                   # designed cases: no placement nearer to collinear than this
SHIFT = (500.0, -800.0, 1200.0)
MAX_BELOW_SHARE = 0.01
PI = float(np.pi)


def _rng(seed):
    return np.random.Generator(np.random.PCG64(int(seed)))


# =====================================================================================================================
# 1. ic -> xyz
# =====================================================================================================================
def _sine(atom1, atom2, atom3):
    """|a x b| / (|a| |b|) of _place's own a and b (the +1e-8 on exact zeros included)."""
    a = atom2 - atom1
    b = atom2 - atom3
    a = torch.where(a == 0.0, a + 1e-8, a)
    b = torch.where(b == 0.0, b + 1e-8, b)
    n = torch.cross(a, b, dim=-1)
    return torch.sqrt((n * n).sum(-1)) / torch.sqrt((a * a).sum(-1) * (b * b).sum(-1))


def chain_xyz_and_sine(og_cg_nxyz, ic, info):
    """oracle/vae_decode.py::ic_to_xyz with the chain sine beside it -> (xyz [B, n_atoms, 3], s [B, n_atoms]), in the
    dtype of the inputs.  The coordinates are those of odec.ic_to_xyz (the same _place calls in the same order)."""
    permute, atom_idx, orders = info
    ca = og_cg_nxyz[:, :, 1:]
    mid, prv, nxt = ca[:, 1:-1], ca[:, :-2], ca[:, 2:]
    one = torch.ones(mid.shape[:2], dtype=ca.dtype)
    N = odec._place(ic[:, :, 0], mid, prv, nxt)
    Cc = odec._place(ic[:, :, 1], mid, nxt, prv)
    O = odec._place(ic[:, :, 2], Cc, mid, N)
    sN, sC = _sine(mid, prv, nxt), _sine(mid, nxt, prv)
    sO = torch.minimum(_sine(Cc, mid, N), torch.minimum(sN, sC))
    atoms = torch.stack((O, N, Cc, mid), dim=2)
    s = torch.stack((sO, sN, sC, one), dim=2)
    B = ca.shape[0]
    for i in range(10):
        def pick(col):
            ix = orders[i, :, col].reshape(1, -1, 1)
            return (torch.gather(atoms, 2, ix.unsqueeze(-1).repeat(B, 1, 1, 3))[:, :, 0],
                    torch.gather(s, 2, ix.repeat(B, 1, 1))[:, :, 0])
        (p2, s2), (p1, s1), (p0, s0) = pick(2), pick(1), pick(0)
        new = odec._place(ic[:, :, 3 + i], p2, p1, p0)
        s_new = torch.minimum(torch.minimum(_sine(p2, p1, p0), s2), torch.minimum(s1, s0))
        atoms = torch.cat([atoms, new.unsqueeze(2)], dim=2)
        s = torch.cat([s, s_new.unsqueeze(2)], dim=2)
    return atoms.reshape(B, -1, 3)[:, atom_idx, :][:, permute, :], s.reshape(B, -1)[:, atom_idx][:, permute]


def synthetic_ic(B, L, seed):
    """Bonds 1.5 +- 0.1, angles 1.9 +- 0.5, torsions N(0, 1) (test_ic_to_xyz_groups_equals_one_launch_per_protein)."""
    return (synth.gaussian((B, L, 13, 3), seed) * torch.tensor([0.1, 0.5, 1.0]) + torch.tensor([1.5, 1.9, 0.0])).float()


def protein_of(z_interior, seed, B):
    """A synthetic protein with the given interior residue types (flanked by ALA)."""
    z_full = np.concatenate([[2], np.asarray(z_interior, dtype=np.int64), [2]])
    full = synth.ca_trace(len(z_full), 1000 + seed)
    return {"xyz_full": synth.perturb_frames(full, B, 3000 + seed), "z_full": z_full, "info": synth.make_info(z_full),
            "n_cg": len(z_interior)}


def og_of(prot):
    z = torch.from_numpy(prot["z_full"]).float()
    x = torch.from_numpy(prot["xyz_full"]).float()
    return torch.cat([z[None, :, None].expand(x.shape[0], -1, 1), x], dim=-1).contiguous()


def _xyz_case(name, prot, ic, designed=True, og=None, **aim):
    og = og_of(prot) if og is None else og
    B, L = ic.shape[0], ic.shape[1]
    assert og.shape == (B, L + 2, 4) and ic.shape == (B, L, 13, 3) and og.dtype == ic.dtype == torch.float32
    return dict(name=name, og=og.contiguous(), ic=ic.contiguous(), info=prot["info"], z=prot["z_full"][1:-1],
                designed=designed, **aim)


def leaf_slots(z_interior):
    """bool [L, 13]: slots (N, C, O, side chain 0..9 in ic order) no other placement of the residue is built from.  A
    multiple of pi as a leaf's bond angle, or a leaf's 1e-3 A bond, spoils no later placement."""
    leaf = np.zeros((len(z_interior), 13), dtype=bool)
    for r, z in enumerate(z_interior):
        nm = synth.IDX2THR[int(z)]
        orders = synth.atom_order_list[nm]
        used = {1, 2, 3} | {int(k) for trip in orders for k in trip}          # O is built from C, CA and N
        if 0 not in used:
            leaf[r, 2] = True                                                # ic row 2 is O (slot 0)
        for i in range(len(orders)):
            leaf[r, 3 + i] = (4 + i) not in used
    return leaf


ANGLE_SPECIALS = (0.0, PI, PI / 2, -PI / 2, 2 * PI, -3 * PI, 7 * PI, -7 * PI, 50.0, -50.0)


def angles_case():
    """Bond angles and torsions from {0 +- 0.05, pi +- 0.05, +-pi/2, 2 pi, -3 pi, +-7 pi, +-50} mixed with ordinary values;
    negative bond lengths anywhere, 1e-3 A bonds and exact multiples of pi as BOND angles on leaf atoms only (on any other
    atom they would make the next placement exactly collinear: 0/0 in the reference too); 0 +- 0.05 and pi +- 0.05 keep
    0.01 away from the multiple for the same reason.  Torsions take every special value everywhere."""
    prot = synth.make_protein(60, 61, n_frames=2, phospho=True)
    B, L = 2, 60
    r = _rng(6101)
    ic = synthetic_ic(B, L, 6102).numpy()
    leaf = np.broadcast_to(leaf_slots(prot["z_full"][1:-1]), (B, L, 13))

    def near(centre, size):
        return centre + r.choice([-1.0, 1.0], size) * r.uniform(0.01, 0.05, size)

    for ch in (1, 2):
        pick = r.uniform(size=(B, L, 13)) < 0.5
        kind = r.integers(0, len(ANGLE_SPECIALS) + 2, size=(B, L, 13))
        val = np.array(ANGLE_SPECIALS + (0.0, PI))[kind]
        val = np.where(kind == len(ANGLE_SPECIALS), near(0.0, kind.shape), val)
        val = np.where(kind == len(ANGLE_SPECIALS) + 1, near(PI, kind.shape), val)
        if ch == 1:                     # a bond angle that is a multiple of pi: leaves only
            multiple = np.isin(kind, (0, 1, 4, 5, 6, 7))
            pick &= ~multiple | leaf
        ic[..., ch] = np.where(pick, val, ic[..., ch])
    ic[..., 0] = np.where(r.uniform(size=(B, L, 13)) < 0.3, -ic[..., 0], ic[..., 0])
    ic[..., 0] = np.where(leaf & (r.uniform(size=(B, L, 13)) < 0.3), 1e-3, ic[..., 0])
    return _xyz_case("angles", prot, torch.from_numpy(ic.astype(np.float32)))


def zero_component_case():
    """Three CA traces of 24 residues whose consecutive differences have exactly zero components (the `== 0 ? + 1e-8`
    branch of place_atom): a walk in the plane z = 5, a staircase of axis-parallel 3.8 A steps, and a walk whose
    residues share their x coordinate in pairs."""
    L, r = 24, _rng(6201)
    prot = protein_of(r.integers(0, 20, L), 62, 3)
    t = np.zeros((3, L + 2, 3), dtype=np.float32)
    ang = np.cumsum(r.choice([-1.0, 1.0], L + 2) * r.uniform(0.3, 1.2, L + 2))
    t[0, :, 0], t[0, :, 1], t[0, :, 2] = np.cumsum(3.8 * np.cos(ang)), np.cumsum(3.8 * np.sin(ang)), 5.0
    for k in range(1, L + 2):
        t[1, k] = t[1, k - 1]
        t[1, k, (k - 1) % 3] += np.float32(3.8)
    step = r.standard_normal((L + 2, 3))
    step[1::2, 0] = 0.0                                                    # residue 2k + 1 keeps the x of residue 2k
    step *= 3.8 / np.linalg.norm(step, axis=1, keepdims=True)
    t[2] = np.cumsum(step, 0).astype(np.float32)
    for f in range(3):
        d = np.diff(t[f], axis=0)
        assert (d == 0).any(), f
    prot["xyz_full"] = t
    return _xyz_case("zero_component", prot, synthetic_ic(3, L, 6202))


def far_case():
    """synth L46 x 3 translated by SHIFT; `near` is the untranslated case."""
    near = synth_case(46, 3)
    og = near["og"].clone()
    og[:, :, 1:] += torch.tensor(SHIFT)
    prot = dict(info=near["info"], z_full=np.concatenate([[2], near["z"], [2]]))
    return _xyz_case("far", prot, near["ic"], og=og, near="synth_L46x3")


def synth_case(L, B):
    return _xyz_case(f"synth_L{L}x{B}", synth.make_protein(L, 70 + L, n_frames=B), synthetic_ic(B, L, 280 + L))


def golden_case(name):
    """A shipped decoder geometry with the internal coordinates an untrained decoder emitted for it (golden g5)."""
    L, B, seed, vae_type = cases.DECODER_CASES[name]
    prot, batch, _latent, _dataname = cases.decoder_inputs(L, B, seed, vae_type)
    ic = torch.from_numpy(np.load(cases.npz_path(f"g5_decode_{name}"))["ic_recon"]).reshape(B, L, 13, 3).float()
    return _xyz_case(name, prot, ic, designed=False, og=batch["OG_CG_nxyz"].reshape(B, L + 2, 4).float())


ROWS = ((1, 1), (2, 1), (1, 127), (1, 128), (1, 129), (3, 43))          # (B, L): B x L = 1, 2, 127, 128, 129, 3 x 43


def rows_case(B, L):
    return _xyz_case(f"rows_{B}x{L}", synth.make_protein(L, 300 + L, n_frames=B), synthetic_ic(B, L, 310 + 7 * L + B))


def table_case(kind):
    """all_types: the 22 residue types of synth (TPO and SEP among them) twice over; gly: a run of GLY (slot_to_out is -1
    for the whole side chain); trp_arg: alternating TRP / ARG (the full chain depth)."""
    idx = synth.IDX2THR.index
    z = {"all_types": list(range(22)) * 2, "gly": [idx("GLY")] * 12, "trp_arg": [idx("TRP"), idx("ARG")] * 6}[kind]
    seed = 400 + len(kind)
    return _xyz_case(kind, protein_of(z, seed, 2), synthetic_ic(2, len(z), seed + 50))


XYZ_CASES = (list(cases.DECODER_CASES) + ["synth_L46x3", "synth_L129x2", "angles", "zero_component", "far"]
             + [f"rows_{B}x{L}" for B, L in ROWS] + ["all_types", "gly", "trp_arg"])


@functools.lru_cache(maxsize=None)
def xyz_case(name):
    if name in cases.DECODER_CASES:
        return golden_case(name)
    if name.startswith("synth_L"):
        L, B = name[len("synth_L"):].split("x")
        return synth_case(int(L), int(B))
    if name.startswith("rows_"):
        B, L = name[len("rows_"):].split("x")
        return rows_case(int(B), int(L))
    if name in ("all_types", "gly", "trp_arg"):
        return table_case(name)
    return {"angles": angles_case, "zero_component": zero_component_case, "far": far_case}[name]()


_xyz_refs = {}


def xyz_reference(case):
    """{x64, s, x32, e_ref, floor, scale} of an ic -> xyz case, computed once and left unchanged.  scale = max(e_ref, floor):
    the rule is err x s <= C x scale."""
    if case["name"] not in _xyz_refs:
        x64, s = chain_xyz_and_sine(case["og"].double(), case["ic"].double(), case["info"])
        x32 = odec.ic_to_xyz(case["og"], case["ic"], case["info"])
        assert x64.dtype == s.dtype == torch.float64 and x32.dtype == torch.float32
        e_ref = float(((x32.double() - x64).norm(dim=-1) * s).max())
        floor = FLOOR_ULP * float(x64.abs().max())
        _xyz_refs[case["name"]] = dict(x64=x64, s=s, x32=x32, e_ref=e_ref, floor=floor, scale=max(e_ref, floor))
    return _xyz_refs[case["name"]]


def worst_atom(xyz, x64, s, scale):
    """-> (ratio, frame, atom, err, s): err x s / scale where it is largest."""
    err = (xyz.double() - x64).norm(dim=-1)
    ratio = err * s / scale
    f, a = divmod(int(ratio.argmax()), ratio.shape[1])
    return float(ratio.max()), f, a, float(err[f, a]), float(s[f, a])


# --- groups ----------------------------------------------------------------------------------------------------------
GROUP_LISTS = ("one_row", "same_protein_twice", "three_total_128", "seventeen")


@functools.lru_cache(maxsize=None)
def group_list(name):
    """-> list of ic -> xyz cases that go into ONE launch of codlad_ic_to_xyz_groups."""
    def g(B, L, k):
        c = rows_case(B, L)
        c["name"] = f"{name}[{k}]_{B}x{L}"
        return c
    if name == "one_row":
        return [g(1, 1, 0)]
    if name == "same_protein_twice":                   # one protein (one info, one trace), two sets of internal coordinates
        a = g(1, 46, 0)
        b = dict(a, name=f"{name}[1]_1x46", ic=synthetic_ic(1, 46, 999))
        return [a, b]
    if name == "three_total_128":                      # 1 + 86 + 41 rows: exactly one full block
        return [g(1, 1, 0), g(2, 43, 1), g(1, 41, 2)]
    shapes = [(1, 1), (1, 7), (1, 1), (2, 43), (3, 12), (1, 1), (1, 22), (2, 5), (1, 46), (1, 1), (3, 3), (1, 2), (2, 12),
              (1, 1), (1, 30), (2, 9), (1, 1)]
    assert len(shapes) == 17
    return [g(B, L, k) for k, (B, L) in enumerate(shapes)]


# =====================================================================================================================
# 2. xyz -> ic
# =====================================================================================================================
def _quad_atoms(xyz, quads):
    ok = (np.asarray(quads) >= 0).all(-1)
    q = np.where(ok[:, None], quads, 0)
    return ok, [xyz[:, q[:, k]] for k in range(4)]


def ic_reference(xyz, quads):
    """-> (ic64 [F, Q, 3], tol [F, Q, 3], ok [Q], collinear [F, Q]) from the float32 frames: oracle/ic_build.py in float64
    and the per-quad tolerances of the module docstring.  collinear: a bond angle of the quad is exactly 0 or pi, its
    dihedral undefined."""
    x = np.asarray(xyz, dtype=np.float64)
    ic64 = ic_build.xyz_to_ic(x, quads)
    ok, (a1, a2, a3, a4) = _quad_atoms(x, quads)
    with np.errstate(invalid="ignore", divide="ignore"):
        amax = np.max(np.abs(np.stack([a1, a2, a3, a4])), axis=(0, -1))
        bonds = np.stack([np.linalg.norm(a1 - a2, axis=-1), np.linalg.norm(a3 - a2, axis=-1), np.linalg.norm(a4 - a3, axis=-1)])
        u = np.maximum(FLOOR_ULP * amax / bonds.min(0), FLOOR_ULP)
        s1, s2 = np.sin(ic_build.angle_between(a1 - a2, a3 - a2)), np.sin(ic_build.angle_between(a2 - a3, a4 - a3))
        smin = np.minimum(s1, s2)
        tol = np.stack([C * FLOOR_ULP * amax, C * u, C * u / smin], axis=-1)
    return ic64, tol, ok, smin < 1e-12


def ic_error(got, ic64):
    d = np.abs(np.asarray(got, dtype=np.float64) - ic64)
    d[..., 1:] = np.minimum(d[..., 1:], 2 * np.pi - d[..., 1:])          # 0 and 2 pi are the same angle
    return d


def hold_ic(label, got, xyz, quads, labels=None):
    """Assert the per-quad tolerances on `got` [F, Q, 3]: distance and bond angle on every present quad, the dihedral where
    it is defined, exact zeros on absent quads.  -> worst err / tol per channel."""
    ic64, tol, ok, collinear = ic_reference(xyz, quads)
    got = np.asarray(got)
    assert got.shape == ic64.shape and np.isfinite(got[:, ok][..., :2]).all()
    err = ic_error(got, ic64)
    assert (got[:, ~ok] == 0).all(), f"{label}: an absent quad is not exactly zero"
    worst = []
    for ch in range(3):
        keep = np.broadcast_to(ok[None], err.shape[:2]) & (~collinear if ch == 2 else True)
        with np.errstate(invalid="ignore", divide="ignore"):
            ratio = np.where(keep, err[..., ch] / tol[..., ch], 0.0)
        assert not np.isnan(ratio).any(), f"{label}: channel {ch} is not a number somewhere"
        f, q = np.unravel_index(int(ratio.argmax()), ratio.shape)
        worst.append(float(ratio.max()))
        what = f" ({labels[q]})" if labels else ""
        assert ratio.max() <= 1.0, (f"{label}: channel {ch} quad {q}{what} frame {f}: err {err[f, q, ch]:.3e} > tol "
                                    f"{tol[f, q, ch]:.3e}")
    return worst


def ic_fp32(xyz, quads, form="atan2"):
    """float32 numpy restatement of xyz_to_ic_kernel, operation by operation; form "arccos": the bond angle as the
    reference states it (arccos of the clipped dot product of the unit vectors) instead."""
    f = np.float32
    x = np.asarray(xyz, dtype=f)
    ok, (p0, p1, p2, p3) = _quad_atoms(x, quads)
    dot = lambda a, b: (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]      # noqa: E731
    cross = lambda a, b: np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],  # noqa: E731
                                   a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)
    with np.errstate(invalid="ignore", divide="ignore"):
        u, w = p0 - p1, p2 - p1
        nu, nw = np.sqrt(dot(u, u)), np.sqrt(dot(w, w))
        if form == "atan2":
            uxw = cross(u, w)
            angle = np.arctan2(np.sqrt(dot(uxw, uxw)), dot(u, w))
        else:
            angle = np.arccos(np.clip(dot(u / nu[..., None], w / nw[..., None]), f(-1), f(1)))
        b0, b2, b1 = u, p3 - p2, w / nw[..., None]
        d0, d2 = dot(b0, b1), dot(b2, b1)
        v, ww = b0 - b1 * d0[..., None], b2 - b1 * d2[..., None]
        tor = np.arctan2(dot(cross(b1, v), ww), dot(v, ww))
        two_pi = f(6.283185307179586)
        tor = np.fmod(tor, two_pi)
        tor = np.where(tor < 0, tor + two_pi, tor)
    out = np.stack([nu, angle, tor], -1).astype(f)
    assert out.dtype == f and u.dtype == f
    out[:, ~ok] = 0
    return out


def _rot_x(p, phi):
    c, s = np.cos(phi), np.sin(phi)
    return np.array([p[0], c * p[1] - s * p[2], s * p[1] + c * p[2]])


@functools.lru_cache(maxsize=None)
def designed_quads():
    """One hand-made frame -> dict(xyz float32 [1, n, 3], quads int32 [Q, 4], label [Q], first_far).  Every quad has four
    atoms of its own, A2 at the origin and A3 at (1.5, 0, 0) (the quads overlap in space: a z offset would swallow the 1e-6
    that makes a dihedral 0+ or 0-); the second half is the first translated by SHIFT."""
    atoms, quads, labels = [], [], []

    def add(label, p0, p3, neg=None):
        k = len(atoms)
        atoms.extend([np.asarray(p0, float), np.zeros(3), np.array([1.5, 0.0, 0.0]), np.asarray(p3, float)])
        q = [k, k + 1, k + 2, k + 3]
        if neg is not None:
            q[neg] = -1
        quads.append(q)
        labels.append(label)

    p3 = (2.0, 1.2, 0.3)
    add("angle_0", (0.75, 0, 0), p3)                                   # A1 on the A2 -> A3 ray: exactly 0
    add("angle_pi", (-1.25, 0, 0), p3)                                 # exactly pi
    for lab, th in (("angle_1e-4", 1e-4), ("angle_pi-1e-4", PI - 1e-4)):
        add(lab, (1.3 * np.cos(th), 1.3 * np.sin(th), 0), p3)
    p0 = (-0.5, 1.2, 0.0)
    for lab, phi in (("dihedral_0+", 1e-6), ("dihedral_0-", -1e-6), ("dihedral_0", 0.0), ("dihedral_+pi", PI),
                     ("dihedral_pi-", PI - 1e-6), ("dihedral_pi+", -PI + 1e-6), ("dihedral_+pi/2", PI / 2),
                     ("dihedral_-pi/2", -PI / 2)):
        add(lab, p0, np.array([1.5, 0, 0]) + _rot_x(np.array([0.5, 1.2, 0.0]), phi))
    add("negative_index", p0, p3, neg=2)
    add("ordinary", p0, (2.1, -0.7, 0.9))
    n = len(quads)
    xyz = np.concatenate([np.array(atoms), np.array(atoms) + np.array(SHIFT)]).astype(np.float32)
    far = [[i + 4 * n if i >= 0 else -1 for i in q] for q in quads]
    return dict(xyz=xyz[None], quads=np.array(quads + far, dtype=np.int32), label=labels + [l + "_far" for l in labels],
                first_far=n)


@functools.lru_cache(maxsize=None)
def golden_frames(name):
    """(Topology with the CA-only flanking residues, full frames [B, n_atoms + 2, 3] float32, og [B, L + 2, 4], info) of a
    shipped decoder geometry: the all-atom coordinates the reference's ic_to_xyz produced (golden g6)."""
    L, B, seed, vae_type = cases.DECODER_CASES[name]
    prot, batch, _latent, _dataname = cases.decoder_inputs(L, B, seed, vae_type)
    gold = np.load(cases.npz_path(f"g6_xyz_{name}"))["xyz"]
    names = [synth.IDX2THR[int(z)] for z in prot["z_full"]]
    atom_names = [["CA"]] + [synth.PDB_ATOM_ORDER[n] for n in names[1:-1]] + [["CA"]]
    og = batch["OG_CG_nxyz"].reshape(-1, L + 2, 4).float()
    full = np.concatenate([og[:, :1, 1:].numpy(), gold, og[:, -1:, 1:].numpy()], 1).astype(np.float32)
    return db.Topology(names, atom_names), full, og, prot["info"]


THREAD_COUNTS = ((3, 85), (2, 128), (1, 257))                          # n_frames x n_quads = 255, 256, 257


_rt_refs = {}


def round_trip_reference(name):
    """The golden frames through xyz -> ic -> xyz.  -> dict(x0 float64 [B, n_atoms, 3] the original coordinates, s the
    chain sine of their float64 internal coordinates, e_ref the fp32 oracle's own round trip (ic_fp32, then
    odec.ic_to_xyz in float32) in err x s, floor, scale)."""
    if name not in _rt_refs:
        top, full, og, info = golden_frames(name)
        B, L = og.shape[0], og.shape[1] - 2
        quads = db.ic_quads(top)
        ic64 = torch.from_numpy(ic_build.xyz_to_ic(full, quads)).reshape(B, L, 13, 3)
        x64, s = chain_xyz_and_sine(og.double(), ic64, info)
        x0 = torch.from_numpy(full[:, 1:-1]).double()
        assert float((x64 - x0).abs().max()) < 1e-9                    # the float64 round trip is the identity
        ic32 = torch.from_numpy(ic_fp32(full, quads)).reshape(B, L, 13, 3)
        x32 = odec.ic_to_xyz(og, ic32, info)
        assert x32.dtype == torch.float32
        e_ref = float(((x32.double() - x0).norm(dim=-1) * s).max())
        floor = FLOOR_ULP * float(x0.abs().max())
        _rt_refs[name] = dict(x0=x0, s=s, e_ref=e_ref, floor=floor, scale=max(e_ref, floor), quads=quads, full=full, og=og,
                              info=info)
    return _rt_refs[name]


# =====================================================================================================================
# 3. decisions
# =====================================================================================================================
def sqrt32(v):
    """The correctly rounded float32 square root (through float64: 53 >= 2 x 24 + 2 bits, so the second rounding is
    innocuous).  torch.sqrt on float32 CPU tensors is not: 12 of the clash job's 2002 sums come out one ulp low on one
    machine and more on another, so a decision of the project's torch oracles within an ulp of a threshold depends on the
    CPU.  The device's sqrtf is the IEEE one; so is the fp32 oracle the rules below compare with inside the margin."""
    assert v.dtype == torch.float32
    return torch.sqrt(v.double()).float()


def dist32(x):
    """[n, n] float32 distances as the kernels form them: sqrt((dx dx + dy dy) + dz dz), operation by operation."""
    x = x.float()
    sq = [(x[:, None, k] - x[None, :, k]) ** 2 for k in range(3)]
    return sqrt32((sq[0] + sq[1]) + sq[2])


def mixed(flagged, dec32, dec64):
    """The decision the device must give: float64's outside the margin, the fp32 oracle's inside."""
    return torch.where(flagged, dec32, dec64)


# --- VQ --------------------------------------------------------------------------------------------------------------
VQ_SIZES = (1, 5, 15, 16, 17, 255, 4095, 4096, 4097, 9000)
VQ_N = (1, 63, 64, 65, 1000)
VQ_SCALES = (1.0, 5.0, 50.0)
VQ_MEAN, VQ_STD = (0.3, -1.1, 0.7), (1.7, 0.6, 2.3)
VQ_WAVES = 16
# (codebook size, first, second index of a duplicated code, what it aims at)
VQ_TIES = ((4096, 300, 400, "inside the range of wave 1"), (4096, 10, 3000, "across the ranges of waves 0 and 11"),
           (4097, 3900, 4090, "inside the last, shorter range"), (17, 16, 3, "the one-code range of wave 8 against wave 1"))


@functools.lru_cache(maxsize=None)
def vq_codebook(size):
    """The first `size` rows of the synthetic N6 codebook, Gaussian rows of the same scale beyond its 4096."""
    cb = odec.codebook_of(synth.vqvae_state_dict("N6", "PED", cases.VAE_SEED)).clone()
    if size > cb.shape[0]:
        mean, std = synth.norm_stats("PED", "N6")
        cb = torch.cat([cb, synth.gaussian((size - cb.shape[0], 3), 7700 + size) * std + mean])
    return cb[:size].contiguous()


def vq_state_dict(codebook):
    sd = synth.vqvae_state_dict("N6", "PED", cases.VAE_SEED)
    sd["quantize._codebook.embed"] = codebook[None].clone()
    return sd


def vq_wave_ranges(size):
    per = (size + VQ_WAVES - 1) // VQ_WAVES
    return [(min(w * per, size), min(min(w * per, size) + per, size)) for w in range(VQ_WAVES)]


def vq_inputs(n, scale, seed):
    """Normalised latents x [n, 3] whose de-normalised values are Gaussian of the given scale (around the codebook)."""
    return (synth.gaussian((n, 3), seed) * scale).float()


def vq_denormalise(x):
    """x * std + mean, the product and the sum rounded separately (eager float32 ops)."""
    return x * torch.tensor(VQ_STD) + torch.tensor(VQ_MEAN)


def vq_reference(latent, codebook):
    """The float64 decision from the float32 latents `latent` (the device's own latent_out) -> (idx64 [n] first index of the
    minimum, flagged [n] margin to the next DISTINCT distance <= 8 x 2^-24 x (|z|^2 + |e1|^2), idx32 the fp32 oracle's)."""
    z, e = latent.reshape(-1, 3).double(), codebook.double()
    d = (z ** 2).sum(1, keepdim=True) + (e ** 2).sum(1) - 2.0 * z @ e.t()
    idx64 = torch.argmin(d, dim=1)
    best = d.gather(1, idx64[:, None])
    dup = (e[None, :, :] == e[idx64][:, None, :]).all(-1)               # exact copies of the winner: ties, not margins
    nxt = torch.where(dup, torch.full_like(d, float("inf")), d).amin(1)
    bound = 8 * 2.0 ** -24 * ((z ** 2).sum(1) + (e[idx64] ** 2).sum(1))
    first_dup = torch.argmax(dup.to(torch.int8), dim=1)
    assert torch.equal(first_dup, idx64)                                 # argmin returns the first of equal minima
    idx32 = odec.vq_lookup(latent.reshape(-1, 3).float(), codebook)[1]
    return idx64, (nxt - best[:, 0]) <= bound, idx32


def vq_tie_inputs(codebook, i, j, n=96, seed=0):
    """Normalised latents whose de-normalised values lie within 1e-3 of the duplicated code: the copies at i and j are
    at exactly the same distance from each, and nothing else is near."""
    z = codebook[i][None] + synth.gaussian((n, 3), 7800 + seed) * 1e-3
    return ((z - torch.tensor(VQ_MEAN)) / torch.tensor(VQ_STD)).float()


def vq_tie_codebook(size, i, j):
    cb = vq_codebook(size).clone()
    cb[j] = cb[i]
    return cb


# --- CG graph --------------------------------------------------------------------------------------------------------
CG_SAMPLES = (1, 2, 63, 64, 65, 128, 129, 300)
CG_CUTOFFS = (21.0, 8.0)


@functools.lru_cache(maxsize=None)
def cg_job():
    """One job: samples of CG_SAMPLES residues, the 65-residue trace once more as a sample of its own (the two copies must
    not see each other), and per cutoff a planted sample of four beads on the x axis at 0, cutoff, the float32 above and
    the float32 below it.  -> dict(xyz [M, 3], lens, planted {cutoff: first node})."""
    xyzs = [torch.from_numpy(synth.make_protein(L, 500 + L)["xyz_full"][0, 1:-1]) for L in CG_SAMPLES]
    xyzs.append(xyzs[CG_SAMPLES.index(65)].clone())
    planted = {}
    for c in CG_CUTOFFS:
        c32 = np.float32(c)
        p = np.zeros((4, 3), dtype=np.float32)
        p[1:, 0] = [c32, np.nextafter(c32, np.float32(np.inf)), np.nextafter(c32, np.float32(0))]
        planted[c] = sum(x.shape[0] for x in xyzs)
        xyzs.append(torch.from_numpy(p))
    lens = [x.shape[0] for x in xyzs]
    assert sum(lens) % 4 != 0
    return dict(xyz=torch.cat(xyzs).float().contiguous(), lens=lens, planted=planted)


def cg_reference(job, cutoff):
    """-> (want [M, M] bool adjacency the device must give, flagged [M, M], stats).  Within a sample: float64 distance <=
    cutoff outside the margin |d64 - cutoff| <= 4 x 2^-23 x cutoff, the fp32 formula (dist32: synth.cg_nbr_list's with a correctly
    rounded sqrt) inside it; the
    planted pairs by the <= rule itself; nothing across samples."""
    x, M = job["xyz"], job["xyz"].shape[0]
    sample = torch.repeat_interleave(torch.arange(len(job["lens"])), torch.tensor(job["lens"]))
    same = (sample[:, None] == sample[None, :]) & ~torch.eye(M, dtype=torch.bool)
    d64 = (x.double()[:, None] - x.double()[None]).pow(2).sum(-1).sqrt()
    in64 = (d64 <= cutoff) & same
    flagged = ((d64 - cutoff).abs() <= C * FLOOR_ULP * cutoff) & same
    in32 = (dist32(x) <= torch.tensor(cutoff, dtype=torch.float32)) & same
    project = torch.zeros(M, M, dtype=torch.bool)                          # the project's own list builder, per sample
    o = 0
    for L in job["lens"]:
        p = synth.cg_nbr_list(x[o:o + L], cutoff) + o
        project[p[:, 0], p[:, 1]] = True
        project[p[:, 1], p[:, 0]] = True
        o += L
    assert bool((project == in32)[~flagged].all())                       # they can differ by torch's sqrt inside the margin only
    want = mixed(flagged, in32, in64)
    p0 = job["planted"][cutoff]
    is_planted = torch.zeros(M, M, dtype=torch.bool)
    for k, inside in ((1, True), (2, False), (3, True)):                 # exactly cutoff: in; above: out; below: in
        for a, b in ((p0, p0 + k), (p0 + k, p0)):
            assert bool(flagged[a, b])
            want[a, b] = inside
            is_planted[a, b] = True
    n_pairs = int(same.sum()) // 2
    below = int((flagged & ~is_planted).sum()) // 2
    return want, flagged, dict(pairs=n_pairs, below=below, planted=3, oracle_ok=bool((in32 == want).all()),
                               fp32_differs_from_fp64=int((in32 != in64).sum()) // 2)


def cg_expected_csr(want):
    """The CSR the device must return for an adjacency: Decoder.csr_from_pairs of its j > i pairs in row-major order."""
    from codlad_amd.engine import Decoder
    nb = torch.nonzero(want)
    return Decoder.csr_from_pairs(nb[nb[:, 1] > nb[:, 0]], want.shape[0])


def cg_adjacency(ptr, src):
    M = ptr.numel() - 1
    recv = torch.repeat_interleave(torch.arange(M), (ptr[1:] - ptr[:-1]).long())
    adj = torch.zeros(M, M, dtype=torch.bool)
    adj[recv, src.long()] = True
    assert int(adj.sum()) == src.numel()                                 # no sender listed twice
    return adj


def cg_order_ok(ptr, src):
    """Per receiver i: the senders j > i ascending, then the senders j < i ascending."""
    for i in range(ptr.numel() - 1):
        s = src[int(ptr[i]):int(ptr[i + 1])].tolist()
        hi, lo = [j for j in s if j > i], [j for j in s if j < i]
        if s != sorted(hi) + sorted(lo):
            return False
    return True


# --- bond graph ------------------------------------------------------------------------------------------------------
BOND_SIZES = (1, 2, 3, 255, 256, 257, 700, 4200)
BOND_ELEMENTS = (1, 6, 7, 8, 16, 15)                                    # H, C, N, O, S, P
BOND_SCALE = 1.3


@functools.lru_cache(maxsize=None)
def bond_job():
    """Structures of BOND_SIZES atoms in ONE call (max_atoms 4200: (4200 + 7) / 8 > 512, the rows loop) and a planted
    structure of four atoms.  Coordinates: the first golden all-atom frame of N6_L46_B3, tiled 60 A apart with a 0.02 A
    jitter per tile; reconstruction = coordinates + 0.1 A noise; elements drawn from H, C, N, O, S, P.
    Planted (C, C, C, H; the H 100 A away): in the reference coordinates atom 1 sits at exactly (r + r) x 1.3 from atom 0
    (`<`: no bond) and atom 2 one float32 below it (bond); the reconstruction swaps the two."""
    r = _rng(8801)
    frame = np.load(cases.npz_path("g6_xyz_N6_L46_B3"))["xyz"][0].astype(np.float32)
    xyz, recon, z = [], [], []
    for n in BOND_SIZES:
        tiles = -(-n // frame.shape[0])
        x = np.concatenate([frame + np.float32(60.0) * np.array([k % 4, (k // 4) % 4, k // 16], dtype=np.float32)
                            + r.standard_normal(frame.shape).astype(np.float32) * np.float32(0.02) for k in range(tiles)])[:n]
        xyz.append(x)
        recon.append(x + r.standard_normal(x.shape).astype(np.float32) * np.float32(0.1))
        z.append(r.choice(BOND_ELEMENTS, size=n))
    cut = (np.float32(gm.COV_CUTOFF[5]) + np.float32(gm.COV_CUTOFF[5])) * np.float32(BOND_SCALE)
    assert cut.dtype == np.float32
    below = np.nextafter(cut, np.float32(0))
    a = np.array([[0, 0, 0], [cut, 0, 0], [0, below, 0], [100, 0, 0]], dtype=np.float32)
    b = np.array([[0, 0, 0], [below, 0, 0], [0, cut, 0], [100, 0, 0]], dtype=np.float32)
    xyz.append(a), recon.append(b), z.append(np.array([6, 6, 6, 1]))
    t = lambda parts: torch.from_numpy(np.concatenate(parts))             # noqa: E731
    return dict(xyz=t(xyz).float(), xyz_recon=t(recon).float(), atomic_nums=t(z).long(),
                num_atoms=list(BOND_SIZES) + [4], planted_counts=[1, 1, 2, 1, 1, 2])


def _dist64(x):
    x = x.double()
    d2 = torch.zeros(x.shape[0], x.shape[0], dtype=torch.float64)
    for k in range(3):
        d2 += (x[:, None, k] - x[None, :, k]) ** 2
    return d2.sqrt_()


def bond_counts(ref, gen, heavy):
    hv = heavy[:, None] & heavy[None, :]
    half = lambda m: int(m.sum()) // 2                                   # noqa: E731
    return [half(ref), half(gen), half(ref != gen), half(ref & hv), half(gen & hv), half((ref != gen) & hv)]


_bond_ref = {}


def bond_reference():
    """Per structure of bond_job(): {want: the six counts the device must give, oracle: the six counts of the fp32 formula
    (oracle/metrics.py::bond_graph's with a correctly rounded sqrt),
    pairs, below: pairs (of either coordinate set) inside the margin |d64 - cut| <= 4 x 2^-23 x cut}.  The float64 cut is
    (r_i + r_j) x scale from the float32 radii and the float32 scale the device is handed."""
    if _bond_ref:
        return _bond_ref["v"]
    job = bond_job()
    table = torch.tensor(gm.COV_CUTOFF, dtype=torch.float32)
    scale = float(np.float32(BOND_SCALE))
    out, o = [], 0
    for n in job["num_atoms"]:
        z = job["atomic_nums"][o:o + n]
        rad = table[z - 1]
        cut = (rad.double()[None, :] + rad.double()[:, None]) * scale
        off = ~torch.eye(n, dtype=torch.bool)
        graphs, g32, below = [], [], 0
        for x in (job["xyz"][o:o + n], job["xyz_recon"][o:o + n]):
            d64 = _dist64(x)
            flagged = ((d64 - cut).abs() <= C * FLOOR_ULP * cut) & off
            b32 = (dist32(x) < (rad[None, :] + rad[:, None]) * torch.tensor(BOND_SCALE, dtype=torch.float32)) & off
            if n <= 700:                    # oracle/metrics.py::bond_graph differs by torch's sqrt inside the margin at most
                assert bool((om.bond_graph(x, rad, BOND_SCALE).bool() == b32)[~flagged].all())
            graphs.append(mixed(flagged, b32, (d64 < cut) & off))
            g32.append(b32)
            below += int(flagged.sum()) // 2
        heavy = z != 1
        out.append(dict(want=bond_counts(graphs[0], graphs[1], heavy), oracle=bond_counts(g32[0], g32[1], heavy),
                        pairs=n * (n - 1), below=below))
        o += n
    _bond_ref["v"] = out
    return out


# --- clash counts ----------------------------------------------------------------------------------------------------
CLASH_THRESHOLD = 1.2
CLASH_EPS = 1e-7


def clash_dist32(x, pairs):
    """The distance as the kernel forms it: sqrt(((dx dx + dy dy) + dz dz) + 1e-7f), float32 operation by operation."""
    d = x[pairs[:, 0]] - x[pairs[:, 1]]
    sq = d * d
    return sqrt32(((sq[:, 0] + sq[:, 1]) + sq[:, 2]) + torch.tensor(CLASH_EPS, dtype=torch.float32))


@functools.lru_cache(maxsize=None)
def clash_job():
    """2000 near pairs (atoms 2k, 2k + 1): 1988 at a distance uniform in 0.9 .. 1.5 A in a random direction, 12 within about
    1e-6 A of 1.2 A, and two planted pairs along x at the float32 separations on either side of the threshold: the largest
    dx whose kernel distance is < 1.2f and the next float32 above it.  -> dict(xyz [n, 3], pairs [n_pairs, 2] sorted,
    planted {pair row: inside})."""
    r = _rng(8901)
    n_pairs = 2000
    first = (r.standard_normal((n_pairs + 2, 3)) * 12.0).astype(np.float32)
    u = r.standard_normal((n_pairs, 3))
    u /= np.sqrt((u[:, 0] ** 2 + u[:, 1] ** 2) + u[:, 2] ** 2)[:, None]         # plain IEEE operations: the same bits anywhere
    dist = r.uniform(0.9, 1.5, n_pairs)
    dist[:12] = CLASH_THRESHOLD + r.uniform(-4e-7, 4e-7, 12)
    second = (first[:n_pairs].astype(np.float64) + u * dist[:, None]).astype(np.float32)
    thr = np.float32(CLASH_THRESHOLD)
    kd = lambda dx: np.sqrt(dx * dx + np.float32(CLASH_EPS), dtype=np.float32)      # noqa: E731
    dx = np.float32(1.1999990)
    while kd(np.nextafter(dx, np.float32(2))) < thr:
        dx = np.nextafter(dx, np.float32(2))
    out_dx = np.nextafter(dx, np.float32(2))
    assert kd(dx) < thr <= kd(out_dx) and dx.dtype == np.float32
    plant_first = np.zeros((2, 3), dtype=np.float32)
    plant_first[1, 1] = 50.0
    plant_second = plant_first.copy()
    plant_second[:, 0] = [dx, out_dx]
    xyz = np.empty((2 * (n_pairs + 2), 3), dtype=np.float32)
    xyz[0::2] = np.concatenate([first[:n_pairs], plant_first])
    xyz[1::2] = np.concatenate([second, plant_second])
    pairs = torch.stack([torch.arange(0, 2 * (n_pairs + 2), 2), torch.arange(1, 2 * (n_pairs + 2), 2)], 1)
    return dict(xyz=torch.from_numpy(xyz), pairs=pairs, planted={n_pairs: True, n_pairs + 1: False})


def clash_reference(job):
    """-> dict(want: the count the device must give, count32 the fp32 formula's, count64, below, planted)."""
    x, p = job["xyz"], job["pairs"]
    thr = float(np.float32(CLASH_THRESHOLD))
    d64 = ((x.double()[p[:, 0]] - x.double()[p[:, 1]]).pow(2).sum(-1) + float(np.float32(CLASH_EPS))).sqrt()
    in64 = d64 < thr
    in32 = clash_dist32(x, p) < torch.tensor(CLASH_THRESHOLD, dtype=torch.float32)
    flagged = (d64 - thr).abs() <= C * FLOOR_ULP * thr
    want = mixed(flagged, in32, in64)
    planted = torch.zeros_like(flagged)
    for row, inside in job["planted"].items():
        assert bool(flagged[row])
        want[row] = inside
        planted[row] = True
    return dict(want=int(want.sum()), count32=int(in32.sum()), count64=int(in64.sum()), below=int((flagged & ~planted).sum()),
                planted_ok=bool((in32[planted] == want[planted]).all()), n=p.shape[0])
