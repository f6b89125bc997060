"""Typed pair-distance histograms on the device (codlad_amd/csrc/pair_hist_kernels.hip through codlad_amd.metrics) against
tests/pair_hist_ref.py.

The counts are integers and the bin decision is a stated float32 sequence: H, over and d_bin EQUAL the float32 restatement,
and lie in the float64 sandwich of tests/test_pair_hist_host.py.  What codlad_pair_hist_profile makes of them is float64 in
one stated order: I, P, I0 and both means equal the numpy restatement to the bit.  Against the exact Debye sum the profile
is held to the derived bound |I - I_debye64| <= 0.43618 q (dr / 2 + delta dr) 2 sum_{i<j} |f_i f_j| (pair_hist_ref.
profile_bound; delta = 4 max |t32 - t64| of the case, reference and restatement only), and Rg^2 I0 to sum |w_i w_j| e (2 r + e),
e = dr / 2 + delta dr (moment_bound), plus the four float64 roundings of the test's own sqrt, square, quotient and product."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from codlad_amd import metrics
from tests import pair_hist_ref as pr
from tests import saxs_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
NAN_KINDS = {"nan": float("nan"), "+inf": float("inf"), "-inf": float("-inf")}


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)                    # a copy: the cached inputs are read-only


def run(key, x=None, types=None):
    c = pr.case(key)
    _n, T, B, dr, _shift = key
    return metrics.pair_histogram_lists(dev(c["x"] if x is None else x), c["types"] if types is None else types, T, dr=dr,
                                        r_max=B * dr)


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


@pytest.mark.gpu
@pytest.mark.parametrize("key", pr.case_keys(), ids=pr.case_id)
def test_counts_equal_the_float32_restatement(key):
    c = pr.case(key)
    n, T, B, dr, _shift = key
    out = run(key)
    H, over, d_bin = (out[k].cpu().numpy() for k in ("H", "over", "d_bin"))
    C = T * (T + 1) // 2
    assert H.dtype == np.int32 and H.shape == (3, C, B) and over.shape == (3, C) and d_bin.shape == (3,)
    assert out["finite"].tolist() == [True] * 3 and out["dr"] == dr
    assert np.array_equal(out["edges"].cpu().numpy(), np.arange(B + 1) * dr) and out["classes"].tolist() == [list(p) for p in pr.classes(T)]
    differ = int((H != c["H32"]).sum())
    print(f"{pr.case_id(key)}: {c['n_pairs']} pairs, delta {c['delta']:.2e} bins, bins that differ from the restatement {differ}, "
          f"pairs beyond the last bin {int(over.sum())}")
    assert np.array_equal(H, c["H32"]) and np.array_equal(over, c["over32"]) and np.array_equal(d_bin, c["d32"])
    for s in range(3):
        assert pr.sandwich(H[s].astype(np.int64), c["cls"], c["t64"][s], c["delta"], B) == 0, s
        for ci, (a, b) in enumerate(pr.classes(T)):                  # the exact invariants
            want = c["count"][a] * c["count"][b] if a < b else c["count"][a] * (c["count"][a] - 1) // 2
            assert int(H[s, ci].sum()) + int(over[s, ci]) == want, (s, a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("key", [(300, 5, 400, 0.5, 0.0), (129, pr.MAX_TYPES, 64, 0.1, 0.0), (65, 1, 64, 0.5, 0.0),
                                 (64, 5, 65, 0.1, 500.0), (2, 1, 1, 0.1, 500.0)], ids=pr.case_id)
def test_bits_repeat_and_depend_on_neither_the_atom_order_nor_the_batch(key):
    c = pr.case(key)
    a, b = run(key), run(key)
    names = ("H", "over", "d_bin", "finite")
    assert all(torch.equal(a[k], b[k]) for k in names)
    rng = np.random.default_rng(17)
    for _ in range(2):                                               # the atoms permuted together with their types
        perm = rng.permutation(key[0])
        p = run(key, c["x"][:, perm], c["types"][perm])
        assert all(torch.equal(a[k], p[k]) for k in names)
    for s in range(3):
        alone = run(key, c["x"][s:s + 1])
        moved = run(key, np.stack([c["x"][(s + 1) % 3], c["x"][(s + 2) % 3], c["x"][s]]))
        first = run(key, np.stack([c["x"][s], c["x"][(s + 1) % 3], c["x"][(s + 2) % 3]]))
        for k in names:
            assert torch.equal(alone[k][0], a[k][s]) and torch.equal(moved[k][2], a[k][s]) and torch.equal(first[k][0], a[k][s])


@pytest.mark.gpu
def test_hand_made_cases():
    def hist(x, types, T, dr=0.5, r_max=8.0):
        return metrics.pair_histogram_lists(dev(np.array(x, dtype=np.float32)[None]), types, T, dr=dr, r_max=r_max)

    def only(h, expect, T):                                          # expect: {(a, b): {bin: count}}
        H = h["H"][0].cpu().numpy()
        want = np.zeros_like(H)
        for (a, b), bins in expect.items():
            for k, v in bins.items():
                want[pr.class_index(a, b, T), k] = v
        return np.array_equal(H, want)

    q = np.array([0.0, 0.1, 0.3])
    # two atoms 1.0 A apart at dr = 0.5: bin 2
    h = hist([[1.0, 2.0, 3.0], [1.0, 3.0, 3.0]], [0, 1], 2)
    assert only(h, {(0, 1): {2: 1}}, 2) and h["d_bin"].tolist() == [2] and int(h["over"].sum()) == 0
    p = metrics.pair_distribution_lists(h, [2.0, 3.0])
    assert p["d_max"].tolist() == [1.5] and p["P"][0].tolist() == [0.0, 0.0, 6.0] + [0.0] * 13 and p["I0"].tolist() == [25.0]
    assert p["rg"].tolist() == [np.sqrt(1.25 * 1.25 * 6.0 / 25.0)] and p["overflow"].tolist() == [False]
    prof = metrics.saxs_profile_hist_lists(h, [[2.0] * 3, [3.0] * 3], q)
    x = q * 1.25
    want = 13.0 + 2.0 * (6.0 * np.where(x == 0, 1.0, np.sin(x) / np.where(x == 0, 1.0, x)))
    assert prof["I"][0].tolist() == want.tolist() and prof["complete"].tolist() == [True]
    # two coincident atoms: bin 0, whichever their types
    for types, T, cls in (([0, 0], 1, (0, 0)), ([1, 0], 2, (0, 1))):
        h = hist([[7.0, 7.0, 7.0], [7.0, 7.0, 7.0]], types, T)
        assert only(h, {cls: {0: 1}}, T) and h["d_bin"].tolist() == [0]
    # a 3-4-5 triangle of three types at dr = 0.5: bins 6, 8, 10
    h = hist([[0.0, 0.0, 0.0], [3.0, 0.0, 0.0], [3.0, 4.0, 0.0]], [2, 0, 1], 3)
    assert only(h, {(0, 2): {6: 1}, (0, 1): {8: 1}, (1, 2): {10: 1}}, 3) and h["d_bin"].tolist() == [10]
    # a pair beyond r_max: counted in `over`, the row of I is NaN and complete = 0, P is still written
    h = hist([[0.0, 0.0, 0.0], [1.2, 0.0, 0.0], [0.0, 9.0, 0.0]], [0, 0, 1], 2)
    assert only(h, {(0, 0): {2: 1}}, 2) and h["over"][0].tolist() == [0, 2, 0] and h["d_bin"].tolist() == [2]
    prof = metrics.saxs_profile_hist_lists(h, [[2.0] * 3, [3.0] * 3], q)
    assert bool(torch.isnan(prof["I"]).all()) and prof["complete"].tolist() == [False] and bool(torch.isnan(prof["mean"]).all())
    p = metrics.pair_distribution_lists(h, [2.0, 3.0])
    assert p["P"][0].tolist() == [0.0, 0.0, 4.0] + [0.0] * 13 and p["overflow"].tolist() == [True] and p["d_max"].tolist() == [1.5]
    assert p["I0"].tolist() == [4.0 + 4.0 + 9.0 + 8.0] and bool(torch.isnan(p["mean"]).all())
    # one atom: no pair, d_bin = -1, d_max = 0 and I = f^2
    h = hist([[3.0, -2.0, 1.0]], [1], 2)
    assert int(h["H"].abs().sum()) == 0 and h["d_bin"].tolist() == [-1] and int(h["over"].sum()) == 0
    prof = metrics.saxs_profile_hist_lists(h, [[2.0, 2.5, 2.25], [3.0, 1.5, 0.5]], q)
    assert prof["I"][0].tolist() == [9.0, 2.25, 0.25] and prof["complete"].tolist() == [True]
    p = metrics.pair_distribution_lists(h, [2.0, 3.0])
    assert p["d_max"].tolist() == [0.0] and p["I0"].tolist() == [9.0] and p["rg"].tolist() == [0.0] and int(p["P"].abs().sum()) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("key", pr.case_keys(), ids=pr.case_id)
def test_profile_and_pair_distribution_equal_the_ordered_restatement(key):
    c = pr.case(key)
    _n, T, B, dr, _shift = key
    h = run(key)
    H, over, d_bin = (h[k].cpu().numpy().astype(np.int64) for k in ("H", "over", "d_bin"))
    finite = np.ones(3, dtype=bool)
    prof = metrics.saxs_profile_hist_lists(h, c["ff"], pr.Q_GRID)
    I_ref, mean_ref, complete = pr.profile_ref(H, over, d_bin, finite, c["count"], c["ff"], pr.sinc_table(pr.Q_GRID, B, dr))
    I, mean = prof["I"].cpu().numpy(), prof["mean"].cpu().numpy()
    assert prof["complete"].tolist() == complete.tolist()
    assert same(I, I_ref) and same(mean, mean_ref)
    r = (np.arange(B) + 0.5) * dr
    p = metrics.pair_distribution_lists(h, c["w"])
    P_ref, I0_ref, m2_ref, meanP_ref = pr.pr_ref(H, over, d_bin, finite, c["count"], c["w"], r * r)
    assert same(p["P"].cpu().numpy(), P_ref) and same(p["mean"].cpu().numpy(), meanP_ref) and same(p["I0"].cpu().numpy(), I0_ref)
    assert same(p["rg"].cpu().numpy(), np.sqrt(m2_ref / I0_ref)) and same(p["d_max"].cpu().numpy(), (d_bin + 1) * dr)
    assert p["overflow"].tolist() == [bool(o.any()) for o in over]
    # I0 = sum_i w_i^2 + 2 sum P, the bins added in ascending order
    wi = c["w"][c["types"]]
    for s in range(3):
        self_term, total = 0.0, 0.0
        for a in range(T):
            self_term = self_term + float(c["count"][a]) * (c["w"][a] * c["w"][a])
        for b in range(int(d_bin[s]) + 1):
            total = total + P_ref[s, b]
        assert p["I0"][s].item() == self_term + 2.0 * total
        assert abs(self_term - (wi * wi).sum()) <= 1e-12 * self_term
    # against the exact Debye sum and the pairwise second moment, where no pair lies beyond the last bin
    ref, _A = sr.debye64(c["x"], c["types"], c["ff"], pr.Q_GRID)
    bound = pr.profile_bound(c["types"], c["ff"], pr.Q_GRID, dr, c["delta"])
    mom = pr.moment_ref(c["x"], c["types"], c["w"])
    rg = p["rg"].cpu().numpy()
    worst = 0.0
    for s in np.nonzero(complete)[0]:
        err = np.abs(I[s] - ref[s])
        assert (err <= bound).all(), (s, (err / np.maximum(bound, 1e-300)).max())
        got = rg[s] * rg[s] * I0_ref[s]
        assert abs(got - mom[s, 0]) <= pr.moment_bound(mom[s, 1], mom[s, 2], dr, c["delta"]) + 4 * 2.0 ** -53 * abs(got), s
        if key[0] > 1:
            worst = max(worst, float((err / bound).max()))
    print(f"{pr.case_id(key)}: complete {complete.tolist()}, max |I - I_debye64| / bound {worst:.4f}")


@pytest.mark.gpu
@pytest.mark.parametrize("n", [4, 129])
def test_non_finite_input_gets_the_defined_result_and_leaves_the_other_structures_alone(n):
    key = (129, pr.MAX_TYPES, 64, 0.1, 0.0)
    c = pr.case(key)
    x, types = c["x"][:, :n], np.minimum(c["types"][:n], 4)
    T, ff, w = 5, c["ff"][:5], c["w"][:5]

    def all_of(xx):
        h = metrics.pair_histogram_lists(dev(xx), types, T, dr=0.5, r_max=40.0)
        return h, metrics.saxs_profile_hist_lists(h, ff, pr.Q_GRID), metrics.pair_distribution_lists(h, w)
    clean = all_of(x)
    assert clean[0]["finite"].tolist() == [True] * 3 and clean[1]["complete"].tolist() == [True] * 3
    assert not bool(torch.isnan(clean[1]["I"]).any()) and not bool(torch.isnan(clean[2]["P"]).any())
    for label, value in NAN_KINDS.items():
        for atom, comps, victim in ((0, (1,), 1), (n // 2, (0, 1, 2), 1), (n - 1, (2,), 1), (n // 2, (1,), 0), (n - 1, (0,), 2)):
            bad = x.copy()
            bad[victim, atom, list(comps)] = value
            h, prof, p = all_of(bad)
            what = (label, atom, comps, victim)
            assert h["finite"].tolist() == [s != victim for s in range(3)] == prof["complete"].tolist(), what
            assert bool((h["H"][victim] == -1).all()) and bool((h["over"][victim] == -1).all()) and int(h["d_bin"][victim]) == -1
            for t in (prof["I"], p["P"], p["I0"], p["rg"], p["d_max"]):
                assert bool(torch.isnan(t[victim]).all()), what
            assert p["overflow"].tolist() == [False] * 3
            others = [s for s in range(3) if s != victim]
            for got, want in zip((h, prof, p), clean):
                for k in ("H", "over", "d_bin", "I", "P", "I0", "rg", "d_max"):
                    if k in got:
                        assert torch.equal(got[k][others], want[k][others]), (what, k)
            mean = np.zeros(pr.Q_GRID.shape[0])
            for s in others:
                mean = mean + clean[1]["I"][s].cpu().numpy()
            assert same(prof["mean"].cpu().numpy(), mean / 2.0), what


@pytest.mark.gpu
def test_buffers_are_written_before_they_are_read_and_only_inside():
    """tests/memcheck.py around the entry points: the results have the same bits under the three fills of every buffer the
    package allocates (H, over, d_bin and the float64 partials among them), every element of every output is written, no
    zone byte changes.  One bin and CODLAD_PAIR_HIST_MAX_BINS of them are among the calls."""
    from codlad_amd.utils.cg_input import template_topology
    from tests.test_buffer_discipline import hold
    c = pr.case((129, 5, 400, 0.5, 0.0))
    top = template_topology(["ALA", "TRP", "GLY", "SEP", "LYS"])
    rng = np.random.default_rng(5)
    xt = (rng.uniform(-8, 8, (3, top.n_atoms, 3))).astype(np.float32)
    xt[1, 3, 0] = np.nan                                             # rows of -1 and of NaN are written rows too

    def case(g):
        out = {}
        for B, dr in ((1, 0.5), (400, 0.5), (4096, 0.0625)):
            h = metrics.pair_histogram_lists(g(torch.from_numpy(c["x"]), "xyz"), c["types"], 5, dr=dr, r_max=B * dr)
            prof = metrics.saxs_profile_hist_lists(h, c["ff"], pr.Q_GRID)
            p = metrics.pair_distribution_lists(h, c["w"])
            for d in (h, prof, p):
                out.update({f"B{B}_{k}": v for k, v in d.items() if torch.is_tensor(v) and k not in ("edges", "classes", "count")})
        x = g(torch.from_numpy(xt), "xyz_top")
        prof, p = metrics.saxs_profile_hist(x, top, r_max=40.0), metrics.pair_distribution(x, top, r_max=40.0)
        for name in [k for k in top.__dict__ if "pair" in k or "hist" in k]:
            top.__dict__.pop(name)                                   # the next fill builds its own tables
        out.update({f"top_{k}": v for k, v in prof.items()})
        out.update({f"top_pr_{k}": v for k, v in p.items()})
        return out, []
    hold("pair_hist", case)


@pytest.mark.gpu
def test_topology_entry_points_cache_their_tables_and_stay_on_the_device():
    from codlad_amd.utils.cg_input import template_topology
    names = ["MET", "ALA", "PRO", "TRP", "GLY", "SER", "LYS", "HIS", "THR", "ARG", "CYS", "ASP", "TYR", "GLN", "GLU", "ASN",
             "ILE", "LEU", "PHE", "VAL"]
    top = template_topology(names)
    groups, types = metrics.saxs_groups(top)
    assert len(groups) == 12
    rng = np.random.default_rng(23)
    x = (rng.uniform(-12, 12, (4, top.n_atoms, 3))).astype(np.float32)
    x[2, 5, 1] = np.inf
    xd = dev(x)
    q = np.linspace(0.01, 0.5, 16)
    h = metrics.pair_histogram(xd, top)
    B = int(np.ceil((3.85 * 20 + 30.0) / 0.5))
    assert tuple(h["H"].shape) == (4, 78, B) and h["finite"].tolist() == [True, True, False, True]
    lists = metrics.pair_histogram_lists(xd, types, 12, dr=0.5, r_max=3.85 * 20 + 30.0)
    assert torch.equal(lists["H"], h["H"]) and torch.equal(lists["d_bin"], h["d_bin"]) and torch.equal(lists["over"], h["over"])
    prof = metrics.saxs_profile_hist(xd, top, q=q)
    p = metrics.pair_distribution(xd, top)
    assert len(top._pair_hist_tables) == 1 and len(top._saxs_hist_tables) == 1 and len(top._pair_distribution_tables) == 1
    # the second call builds nothing and moves nothing between the host and the device
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        h2 = metrics.pair_histogram(xd, top)
        prof2 = metrics.saxs_profile_hist(xd, top, q=q)
        p2 = metrics.pair_distribution(xd, top)
        again = metrics.saxs_profile_hist(None, top, q=q, hist=h2)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert len(top._pair_hist_tables) == 1 and len(top._saxs_hist_tables) == 1 and len(top._pair_distribution_tables) == 1
    assert top._pair_hist_groups == {"n": 12}                        # what a given histogram is checked against
    good = [0, 1, 3]
    for a, b in ((h, h2), (prof, prof2), (p, p2), (prof, again)):
        for k, v in a.items():                                       # per structure: the good rows (NaN is not equal to NaN)
            if torch.is_tensor(v):
                rows = good if v.dim() and v.shape[0] == 4 else slice(None)
                assert torch.equal(v[rows] if v.dim() else v, b[k][rows] if v.dim() else b[k]), k
    assert prof["finite"].tolist() == [True, True, False, True] == prof["complete"].tolist() and int(prof["n_finite"]) == 3
    assert prof["q"].dtype == torch.float32 and np.array_equal(prof["q"].cpu().numpy(), q.astype(np.float32))
    assert p["r"].tolist() == [(b + 0.5) * 0.5 for b in range(B)] and p["overflow"].tolist() == [False] * 4
    # another q grid from the same histogram: the bits of a fresh call on that grid
    q2 = np.linspace(0.0, 0.3, 25)
    second = metrics.saxs_profile_hist(None, top, q=q2, hist=h)
    fresh = metrics.saxs_profile_hist(xd, top, q=q2)
    assert tuple(second["I"].shape) == (4, 25) and len(top._saxs_hist_tables) == 2
    for k in ("q", "mean", "finite", "complete"):
        assert torch.equal(second[k], fresh[k]), k
    assert same(second["I"].cpu().numpy(), fresh["I"].cpu().numpy())
    # within the derived bound of saxs_profile's Debye sum on the same structures (saxs_profile's own float32 error, below
    # 1e-6 of its terms, is not added to the bound: the measured deviation is some hundred times inside it)
    exact = metrics.saxs_profile(xd, top, q=q)["I"].cpu().numpy()
    table = metrics.form_factors(q, groups)
    t = types.astype(np.int64)
    i, j, _c = pr.pair_classes(t, 12)
    delta = 4.0 * max(float(np.abs(pr.t32(x[s], i, j, np.float32(2.0)).astype(np.float64) - pr.t64(x[s], i, j, 0.5)).max()) for s in good)
    bound = pr.profile_bound(t, table, q, 0.5, delta)
    err = np.abs(prof["I"].cpu().numpy()[good] - exact[good])
    print(f"saxs_profile_hist against saxs_profile, {top.n_atoms} atoms: max |difference| / bound {(err / bound).max():.4f}, "
          f"relative to I {(err / np.abs(exact[good])).max():.2e}")
    assert (err <= bound).all() and np.isnan(prof["I"].cpu().numpy()[2]).all()
    # P(r): I0 is the forward scattering, Rg the weighted pairwise one within its bound
    w = metrics.form_factors([0.0], groups)[:, 0]
    mom = pr.moment_ref(x[good], t, w)
    I0 = p["I0"].cpu().numpy()[good]
    assert (np.abs(I0 - w[t].sum() ** 2) <= 1e-9 * I0).all()
    got = p["rg"].cpu().numpy()[good] ** 2 * I0
    assert (np.abs(got - mom[:, 0]) <= pr.moment_bound(mom[:, 1], mom[:, 2], 0.5, delta) + 4 * 2.0 ** -53 * np.abs(got)).all()
    with pytest.raises(ValueError, match="atoms"):
        metrics.pair_histogram(dev(x[:, :-1]), top)
    with pytest.raises(ValueError, match="types"):
        metrics.saxs_profile_hist(None, template_topology(["GLY", "GLY"]), hist=h)


# ---------------------------------------------------------------------------------------------------------------- CLI
def _cli(cwd, *extra, ok=True):
    cmd = [sys.executable, os.path.join(ROOT, "test.py"), "--synthetic", "--synthetic_weights", "--num_sampling_steps", "4",
           "--num_ensemble", "2"] + list(extra)
    res = subprocess.run(cmd, env=dict(os.environ, PYTHONPATH=ROOT), cwd=str(cwd), capture_output=True, text=True, timeout=600)
    assert (res.returncode == 0) == ok, res.stdout[-1500:] + res.stderr[-3000:]
    files = {f: os.path.join(dp, f) for dp, _d, fs in os.walk(os.path.join(str(cwd), "logs")) for f in fs}
    return files, res.stdout, res.stderr


@pytest.mark.gpu
def test_cli_pr_end_to_end(tmp_path):
    from codlad_amd import synth
    from codlad_amd.utils.cg_input import template_topology
    for d in ("on", "refused"):
        (tmp_path / d).mkdir()
    on, stdout, _err = _cli(tmp_path / "on", "--pr", "0.25")
    new = {f for f in on if f.endswith(("_pr.npy", "_pr_r.npy"))}
    assert len(new) == 2 * 4                                         # the four PED-shaped proteins
    assert "pair distribution P(r)" in stdout and "D_max" in stdout and "structures with overflow" in stdout and "pr_rg_mean" in stdout
    i, L = 0, 46
    name = f"synthetic_L{L}"
    xyz = np.load(on[f"{name}_xyz_recon.npy"])
    n_atoms = xyz.shape[2]
    prot = synth.make_protein(L, 1000 + i, n_frames=1)
    top = template_topology([synth.IDX2THR[int(z)] for z in prot["z_full"]][1:-1])
    assert top.n_atoms == n_atoms
    P, r = np.load(on[f"{name}_pr.npy"]), np.load(on[f"{name}_pr_r.npy"])
    B = int(np.ceil((3.85 * L + 30.0) / 0.25))
    assert P.dtype == np.float64 and P.shape == (xyz.shape[0] * xyz.shape[1], B) and r.tolist() == [(b + 0.5) * 0.25 for b in range(B)]
    want = metrics.pair_distribution(dev(xyz.reshape(-1, n_atoms, 3)), top, dr=0.25)
    assert np.array_equal(P, want["P"].cpu().numpy(), equal_nan=True)
    block = next(b for b in stdout.split("vvvvvvvvv pair distribution P(r)")[1:] if f"data_name {name}\n" in b)
    assert float(block.split("pr_overflow ")[1].split()[0]) == float(want["overflow"].sum())
    assert abs(float(block.split("pr_rg_mean ")[1].split()[0]) - float(want["rg"][want["finite"]].mean())) <= 1e-9
    # refused exactly where --observables is
    _files, _out, err = _cli(tmp_path / "refused", "--pr", "--experiment", "bpd", ok=False)
    assert "--pr describes generated structures" in err
