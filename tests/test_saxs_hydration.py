"""The SAXS hydration model on the device (codlad_amd/csrc/saxs_hydration_kernels.hip through codlad_amd.metrics) against
the references of tests/saxs_hydration_ref.py.

The bound of a partial: |P_dev - P_ref| <= 4 * dev32_ab(case) * A_ab[s, k], with A_ab the sum of the absolute terms of the
partial and dev32_ab = max |P_r32 - P_ref| / A_ab, P_r32 the float32 restatement of the header's sequence - reference and
restatement only, nothing of the device's output; 4 is tests/test_saxs.py's MARGIN.  The restatement is operation for
operation the kernel's, so the device is expected at a ratio near 1 and with the restatement's bits; every test prints what
it observed.  The combination and the fit are float64 +, * and / in a stated order: their numpy restatement is held to the
device's bits, not to a tolerance."""
import numpy as np
import pytest
import torch

from codlad_amd import metrics
from tests import saxs_hydration_ref as hr
from tests.test_saxs import MARGIN, NAN_KINDS, _cli, dev

pytestmark = pytest.mark.gpu
C1_GRID, C2_GRID = metrics.default_c1(), metrics.default_c2()
PLANTED = (14, 35)                                                  # c1 = 1.02, c2 = 1.5 on the default grids


def run(c, x=None, weight=None):
    return metrics.saxs_partials_lists(dev(c["x"] if x is None else x), c["types"], c["ff_t"], c["ff_d"],
                                       dev(c["weight"] if weight is None else weight), c["q"])


@pytest.mark.parametrize("key", hr.case_keys(), ids=hr.case_id)
def test_partials_against_float64_the_plain_profile_and_the_combination(key):
    c = hr.case(key)
    out = run(c)
    P = out["P"].cpu().numpy()
    assert P.dtype == np.float64 and P.shape == c["P"].shape and out["finite"].tolist() == [True] * hr.N_STRUCT
    # 1. every partial against float64
    err = np.abs(P - c["P"])
    scale = c["dev32"][None, :, None] * c["A"]
    ratios = [float((err[:, a][scale[:, a] > 0] / scale[:, a][scale[:, a] > 0]).max()) if (scale[:, a] > 0).any() else 0.0 for a in range(6)]
    same = int((P == c["P32"]).sum())
    print(f"{hr.case_id(key)}: dev32 " + " ".join(f"{n} {d:.2e}" for n, d in zip(hr.NAMES, c["dev32"])) + "; max |P_dev - P_ref| / "
          f"(dev32 A) " + " ".join(f"{r:.3f}" for r in ratios) + f"; elements with the restatement's bits {same} of {P.size}")
    assert (err <= MARGIN * scale).all(), (key, np.argwhere(err > MARGIN * scale)[:5].tolist())
    # 2. tt is the plain profile, bit for bit
    plain = metrics.saxs_profile_lists(dev(c["x"]), c["types"], c["ff_t"], c["q"])
    assert torch.equal(out["P"][:, 0], plain["I"])
    # 3. the combination: (1, 0) is P_tt; at (1.03, 2.0) the stated float64 order, and the direct double sum within the bound
    assert torch.equal(metrics.saxs_combine(out["P"], c["q"], c["water"], 1.0, 0.0), out["P"][..., 0, :])
    got = metrics.saxs_combine(out["P"], c["q"], c["water"], 1.03, 2.0).cpu().numpy()
    assert got.shape == (hr.N_STRUCT, key[1]) and np.array_equal(got, hr.combine64(P, c["q"], c["water"], 1.03, 2.0))
    coef = np.abs(hr.coefficients64(c["q"], c["water"], 1.03, 2.0))                  # [6, Q]
    direct = hr.direct64(c["x"], c["types"], c["ff_t"], c["ff_d"], c["weight"], c["q"], c["water"], 1.03, 2.0)
    n = key[0]
    # the float32 share, and the float64 roundings of the reference's n (n + 1) / 2 terms and of the six-term combination
    bound = (coef[None] * (MARGIN * scale + 2.0 ** -53 * (n * (n + 1) / 2 + 16) * c["A"])).sum(1)
    worst = float((np.abs(got - direct) / np.where(bound > 0, bound, 1.0)).max())
    print(f"  I(1.03, 2.0) against the direct sum of |F|^2: max |I_dev - I_ref| / bound {worst:.3f}")
    assert (np.abs(got - direct) <= bound).all()


def _planted_fit():
    c = hr.case(hr.FIT_KEY)
    exp = 3.7 * hr.combine64(c["P"][0], c["q"], c["water"], C1_GRID[PLANTED[0]], C2_GRID[PLANTED[1]])
    sigma = 0.01 * exp + 1e-3 * exp[0]
    return c, exp, sigma


def test_fit_returns_the_planted_grid_point_with_the_restatements_bits():
    c, exp, sigma = _planted_fit()
    assert (C1_GRID[PLANTED[0]], C2_GRID[PLANTED[1]]) == (1.02, 1.5)
    ref = hr.fit64(c["P"][0], c["q"], c["water"], exp, sigma, C1_GRID, C2_GRID)
    order = np.sort(ref["chi2_grid"].reshape(-1))
    print(f"float64 reference: chi2 at the planted point {order[0]:.3e}, the runner-up's {order[1]:.3e}")
    assert ref["index"] == PLANTED[0] * 61 + PLANTED[1] and order[0] < 1e-20 and order[1] > 1e-4
    P = run(c)["P"]
    fit = metrics.saxs_hydration_fit(P[0], c["q"], c["water"], exp, sigma)
    assert int(fit["index"]) == ref["index"] and float(fit["c1"]) == 1.02 and float(fit["c2"]) == 1.5
    own = hr.fit64(P[0].cpu().numpy(), c["q"], c["water"], exp, sigma, C1_GRID, C2_GRID)
    chi2 = fit["chi2_grid"].cpu().numpy()
    print(f"device partials: chi2 at the planted point {float(fit['chi2']):.3e}, scale {float(fit['scale'])!r}")
    assert chi2.shape == (21, 61) and np.array_equal(chi2, own["chi2_grid"])
    assert np.array_equal(fit["scale_grid"].cpu().numpy(), own["scale_grid"])
    assert float(fit["scale"]) == own["scale_grid"][PLANTED] and float(fit["chi2"]) == own["chi2_grid"][PLANTED]
    assert np.array_equal(fit["I"].cpu().numpy(), own["I"]) and abs(float(fit["scale"]) - 3.7) < 1e-4
    # a batch agrees with single calls; an all-NaN set has no best point and leaves the others alone
    batch = torch.stack([P[0], P[1], torch.full_like(P[0], float("nan")), P[2]])
    many = metrics.saxs_hydration_fit(batch, c["q"], c["water"], exp, sigma)
    assert many["index"].dtype == torch.int32 and many["index"].tolist()[2] == -1 and int(many["index"][0]) == ref["index"]
    assert bool(torch.isnan(many["I"][2]).all()) and all(bool(torch.isnan(many[k][2])) for k in ("c1", "c2", "scale", "chi2"))
    for b, s in ((0, 0), (1, 1), (3, 2)):
        one = metrics.saxs_hydration_fit(P[s], c["q"], c["water"], exp, sigma)
        for k in one:
            assert torch.equal(one[k], many[k][b]), (k, b)
    # a planted exact tie: the same c2 twice (and the same c1 twice) - the lowest flat index wins
    tie = metrics.saxs_hydration_fit(P[0], c["q"], c["water"], exp, sigma, c1=[1.0, 1.02, 1.02], c2=[0.5, 1.5, 1.5, 2.0])
    grid = tie["chi2_grid"].cpu().numpy()
    assert grid[1, 1] == grid[1, 2] == grid[2, 1] == grid[2, 2] == grid.min() and int(tie["index"]) == 1 * 4 + 1
    want = hr.fit64(P[0].cpu().numpy(), c["q"], c["water"], exp, sigma, [1.0, 1.02, 1.02], [0.5, 1.5, 1.5, 2.0])
    assert want["index"] == 5 and np.array_equal(grid, want["chi2_grid"])


@pytest.mark.parametrize("key", [(300, 51, 5, 0.0, "plain"), (129, hr.CHUNK + 1, 5, 500.0, "q0"), (65, 51, 5, 0.0, "coincident"),
                                 (2, 1, 1, 500.0, "plain")], ids=hr.case_id)
def test_results_are_bit_identical_and_independent_of_the_batch(key):
    c = hr.case(key)
    a, b = run(c), run(c)
    assert torch.equal(a["P"], b["P"]) and torch.equal(a["finite"], b["finite"])
    for s in range(hr.N_STRUCT):
        alone = run(c, c["x"][s:s + 1], c["weight"][s:s + 1])
        assert torch.equal(alone["P"][0], a["P"][s]), s
        order = [(s + 1) % 3, (s + 2) % 3, s]
        moved = run(c, c["x"][order], c["weight"][order])
        assert torch.equal(moved["P"][2], a["P"][s]), s


@pytest.mark.parametrize("n", [4, 129])
def test_non_finite_input_gets_the_defined_result_and_leaves_the_other_structures_alone(n):
    c = hr.case((129, hr.CHUNK + 1, 5, 500.0, "q0"))
    x, wt, types = c["x"][:, :n], c["weight"][:, :n], c["types"][:n]
    clean = run(c | dict(types=types), x, wt)
    assert clean["finite"].tolist() == [True] * 3 and not bool(torch.isnan(clean["P"]).any())
    for label, value in NAN_KINDS.items():
        for atom, comps, victim in ((0, (1,), 1), (n // 2, (0, 1, 2), 1), (n - 1, (2,), 1), (n // 2, (1,), 0), (n - 1, (0,), 2),
                                    (0, None, 0), (n // 2, None, 1), (n - 1, None, 2)):
            bx, bw = x.copy(), wt.copy()
            if comps is None:
                bw[victim, atom] = value                              # a weight
            else:
                bx[victim, atom, list(comps)] = value                 # a coordinate
            out = run(c | dict(types=types), bx, bw)
            what = (label, atom, comps, victim)
            assert out["finite"].tolist() == [s != victim for s in range(3)], what
            assert bool(torch.isnan(out["P"][victim]).all()) and tuple(out["P"][victim].shape) == (6, hr.CHUNK + 1), what
            for s in range(3):
                if s != victim:
                    assert torch.equal(out["P"][s], clean["P"][s]), (what, s)


def _template():
    from codlad_amd.utils.cg_input import template_topology
    names = ["MET", "ALA", "PRO", "TRP", "GLY", "SEP", "LYS", "HIS", "TPO", "ARG", "CYS", "ASP", "TYR", "GLN"]
    top = template_topology(names)
    x = (np.random.default_rng(11).uniform(-12, 12, (4, top.n_atoms, 3))).astype(np.float32)
    x[2, 5, 1] = np.inf
    return top, x


def test_buffers_are_written_before_they_are_read_and_only_inside():
    """tests/memcheck.py around the four functions: the same bits under the three fills of every buffer the package
    allocates (the workgroups' partials and the exposure among them), every element written, no zone byte changed."""
    from tests.test_buffer_discipline import hold
    c = hr.case((129, hr.CHUNK + 1, 5, 500.0, "q0"))
    top, xt = _template()                                            # structure 2 is not finite: rows of NaN are written rows
    _c, exp, sigma = _planted_fit()
    c300 = hr.case(hr.FIT_KEY)

    def case(g):
        out = metrics.saxs_partials_lists(g(torch.from_numpy(c["x"]), "xyz"), c["types"], c["ff_t"], c["ff_d"],
                                          g(torch.from_numpy(c["weight"]), "weight"), c["q"])
        prof = metrics.saxs_partials(g(torch.from_numpy(xt), "xyz_top"), top)
        for name in ("_saxs_hydration_tables", "_sasa_tables"):
            top.__dict__.pop(name)                                   # the next fill builds its own tables
        I = metrics.saxs_combine(out["P"], c["q"], c["water"], 1.03, 2.0)
        Pf = g(torch.from_numpy(c300["P"][:2]), "P_fit")
        fit = metrics.saxs_hydration_fit(Pf, c300["q"], c300["water"], exp, sigma)
        res = dict(P=out["P"], finite=out["finite"], I=I, prof_P=prof["P"], prof_mean=prof["mean"], prof_finite=prof["finite"],
                   prof_exposure=prof["exposure"], prof_water=prof["water"], prof_q=prof["q"])
        res.update({f"fit_{k}": v for k, v in fit.items()})
        return res, []
    hold("saxs_hydration", case)


def test_saxs_partials_on_a_topology():
    top, x = _template()
    q64 = np.linspace(0.0, 0.5, 51)
    before = metrics.saxs_profile(dev(x), top)
    assert len(top._saxs_tables) == 1
    out = metrics.saxs_partials(dev(x), top, n_points=96)
    assert "_saxs_hydration_tables" in top.__dict__ and len(top._saxs_hydration_tables) == 1 and len(top._saxs_tables) == 1
    assert np.array_equal(out["q"].cpu().numpy(), q64.astype(np.float32))
    assert out["finite"].tolist() == [True, True, False, True] and int(out["n_finite"]) == 3
    area = metrics.sasa(dev(x), top, n_points=96)
    assert out["exposure"].dtype == torch.float32 and torch.equal(out["exposure"], area["exposed"] / 96)
    good = [0, 1, 3]
    assert float(out["exposure"][good].min()) >= 0.0 and float(out["exposure"][good].max()) <= 1.0
    assert out["water"].dtype == torch.float64 and np.array_equal(out["water"].cpu().numpy(), metrics.form_factors(q64, [("O", 2)])[0])
    P = out["P"].cpu().numpy()
    assert P.shape == (4, 6, 51) and np.isnan(P[2]).all() and torch.equal(out["P"][good, 0], before["I"][good])
    # against float64 from the tables the route builds
    groups, types = metrics.saxs_groups(top)
    t = metrics.form_factors(q64, groups)
    d = metrics.form_factors(q64, groups, 0.0) - t
    assert (d > 0).all() and (t < 0).any() and (t > 0).any()
    wt = out["exposure"].cpu().numpy()[good]
    ref, A = hr.partials64(x[good], types, t.astype(np.float32), d.astype(np.float32), wt, out["q"].cpu().numpy())
    r32 = np.stack([hr.partials32(x[s], types, t.astype(np.float32), d.astype(np.float32), wt[k], out["q"].cpu().numpy())
                    for k, s in enumerate(good)])
    dev32 = (np.abs(r32 - ref) / A).max(axis=(0, 2))
    ratio = (np.abs(P[good] - ref) / (dev32[None, :, None] * A)).max()
    print(f"saxs_partials, {top.n_atoms} atoms, {len(groups)} groups: dev32 {dev32.max():.3e}, max ratio {ratio:.3f}, "
          f"mean exposure {wt.mean():.3f}")
    assert (np.abs(P[good] - ref) <= MARGIN * dev32[None, :, None] * A).all()
    mean = np.zeros((6, 51))
    for s in good:                                                   # float64, index order
        mean = mean + P[s]
    assert np.array_equal(out["mean"].cpu().numpy(), mean / 3.0)
    lists = metrics.saxs_partials_lists(dev(x), types, t, d, out["exposure"], q64)
    assert torch.equal(lists["P"][good], out["P"][good])
    # cached once per (q, solvent density, device); the plain route's cache is its own
    metrics.saxs_partials(dev(x), top, n_points=96)
    assert len(top._saxs_hydration_tables) == 1 and len(top._saxs_tables) == 1
    metrics.saxs_partials(dev(x), top, solvent_density=0.3, n_points=96)
    assert len(top._saxs_hydration_tables) == 2 and len(top._saxs_tables) == 1
    none = metrics.saxs_partials(dev(x[2:3]), top, n_points=96)
    assert bool(torch.isnan(none["mean"]).all()) and int(none["n_finite"]) == 0
    # what needs a device tensor to be refused
    with pytest.raises(ValueError, match="atoms"):
        metrics.saxs_partials(dev(x[:, :-1]), top)
    with pytest.raises(ValueError, match=r"weight must be \[S, n_atoms\]"):
        metrics.saxs_partials_lists(dev(x), types, t, d, out["exposure"][:, :-1], q64)
    with pytest.raises(ValueError, match=r"\[6, Q\] or \[B, 6, Q\]"):
        metrics.saxs_hydration_fit(out["P"][None], q64, out["water"], np.ones(51), np.ones(51))
    with pytest.raises(ValueError, match="positive"):
        metrics.saxs_hydration_fit(out["mean"], q64, out["water"], np.ones(51), np.zeros(51))
    with pytest.raises(ValueError, match="c1 must be positive"):
        metrics.saxs_combine(out["mean"], q64, out["water"], 0.0, 1.0)
    # the hydrated profile of the ensemble: the shell adds scattering at q = 0 (every factor of the ts and ss terms is positive there)
    wet = metrics.saxs_combine(out["mean"], out["q"], out["water"], 1.0, 2.0)
    assert tuple(wet.shape) == (51,) and float(wet[0]) > float(out["mean"][0, 0])


def test_cli_saxs_hydration_end_to_end(tmp_path):
    from codlad_amd import synth
    from codlad_amd.utils.cg_input import template_topology
    for d in ("fixed", "plain", "fit"):
        (tmp_path / d).mkdir()
    fixed, stdout = _cli(tmp_path / "fixed", "--saxs", "16", "--saxs_hydration", "1.02", "1.5")
    plain, stdout_plain = _cli(tmp_path / "plain", "--saxs", "16")
    new = {f for f in fixed if f.endswith("_saxs_partials.npy")}
    assert set(fixed) - set(plain) == new and set(plain) <= set(fixed) and len(new) == 4       # the four PED-shaped proteins
    assert "saxs_c1 1.02" in stdout and "saxs_c2 1.5" in stdout and "saxs_c1" not in stdout_plain and "hydrat" not in stdout_plain
    L, name = 46, "synthetic_L46"
    xyz = np.load(fixed[f"{name}_xyz_recon.npy"])
    n_atoms = xyz.shape[2]
    prot = synth.make_protein(L, 1000, n_frames=1)
    top = template_topology([synth.IDX2THR[int(z)] for z in prot["z_full"]][1:-1])
    assert top.n_atoms == n_atoms
    flat = dev(xyz.reshape(-1, n_atoms, 3))
    q64 = np.linspace(0.0, 0.5, 16)
    # without the flag: the parent's code path, bit for bit
    assert np.array_equal(np.load(plain[f"{name}_saxs.npy"]), metrics.saxs_profile(flat, top, q=q64)["I"].cpu().numpy(), equal_nan=True)
    for f in plain:
        if not f.endswith("_saxs.npy"):
            assert open(fixed[f], "rb").read() == open(plain[f], "rb").read(), f             # nothing else changes
    want = metrics.saxs_partials(flat, top, q=q64)
    P, I = np.load(fixed[f"{name}_saxs_partials.npy"]), np.load(fixed[f"{name}_saxs.npy"])
    assert P.dtype == np.float64 and P.shape == (flat.shape[0], 6, 16) and np.array_equal(P, want["P"].cpu().numpy(), equal_nan=True)
    hyd = metrics.saxs_combine(want["P"], want["q"], want["water"], 1.02, 1.5)
    assert I.dtype == np.float64 and I.shape == (flat.shape[0], 16) and np.array_equal(I, hyd.cpu().numpy(), equal_nan=True)
    assert np.array_equal(np.load(fixed[f"{name}_saxs_q.npy"]), q64.astype(np.float32))
    # the fit against a curve written from the run's own mean partials at a planted grid point
    c1, c2 = float(C1_GRID[12]), float(C2_GRID[31])
    curve = 2.0 * metrics.saxs_combine(want["mean"], want["q"], want["water"], c1, c2).cpu().numpy()
    sigma = 0.01 * curve + 1e-3 * curve[0]
    path = tmp_path / "curve.dat"
    path.write_text("# q I sigma\n" + "".join(f"{float(a)!r} {float(b)!r} {float(s)!r}\n" for a, b, s in zip(q64, curve, sigma)))
    fit, out = _cli(tmp_path / "fit", "--saxs", "--saxs_data", str(path), "--saxs_hydration")
    block = next(b for b in out.split("vvvvvvvvv SAXS profile")[1:] if f"data_name {name}\n" in b)
    word = lambda key: float(block.split(key + " ")[1].split()[0])                           # noqa: E731
    print(f"--saxs_hydration fit: c1 {word('saxs_c1')!r} c2 {word('saxs_c2')!r} scale {word('saxs_scale')!r} chi2 "
          f"{word('saxs_chi2')!r}, unhydrated chi2 {word('saxs_chi2_unhydrated')!r}")
    assert (word("saxs_c1"), word("saxs_c2")) == (c1, c2) and abs(word("saxs_scale") - 2.0) < 1e-9
    assert word("saxs_chi2") < 1e-20 < word("saxs_chi2_unhydrated")
    hyd = metrics.saxs_combine(want["P"], want["q"], want["water"], c1, c2)
    assert np.array_equal(np.load(fit[f"{name}_saxs.npy"]), hyd.cpu().numpy(), equal_nan=True)
    assert np.load(fit[f"{name}_saxs_partials.npy"]).shape == (flat.shape[0], 6, 16)
