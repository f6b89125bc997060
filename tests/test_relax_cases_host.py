"""CPU: the designed inputs of tests/relax_cases.py and the conditioning rule are what tests/test_relax_fp64_parity.py takes them
for - decided by the float64 reference and its numpy float32 restatement, before the device sees anything.

Figures of one run (printed): E_ref, the restatement's largest r_a per structure, is 0.15 to 0.86 on the nine cases of
tests/test_relax.py and 0.053 to 0.86 on the designed ones (the lowest: `start`, where only the repulsion has a gradient); its
energies read at most 0.35 / 0.97 / 0.65 of scale_E (distance / torsion / repulsion)."""
import numpy as np

from tests import relax_cases as rc
from tests import relax_ref as rr
from tests import test_relax as tr

F32 = np.float32
ALL = list(rc.CASES)


def all_refs():
    for name in ALL:
        for s, refs in enumerate(rc.get(name)["refs"]):
            for r in refs:
                yield name, s, r
    for n in tr.SIZES:
        for s, refs in enumerate(rc.existing(n)["refs"]):
            yield f"case({n})", s, refs[0]


def test_scale_is_flat_and_the_restatement_keeps_the_energy_scale():
    """E_ref in [0.05, 2] on every structure that has a free atom with a term; every energy of the restatement within scale_E;
    the restatement's r_a of an atom without a term, and of a fixed atom, is 0."""
    lo, hi, worst_e = np.inf, 0.0, np.zeros(3)
    for name, s, r in all_refs():
        free_with_term = ~r["fixed"] & (r["scale"] > 0)
        assert np.isfinite(r["r32"]).all(), (name, s)
        assert not r["r32"][~free_with_term].any(), (name, s)
        assert (r["e32_ratio"] <= 1.0).all(), (name, s, r["e32_ratio"])
        worst_e = np.maximum(worst_e, r["e32_ratio"])
        if free_with_term.any():
            assert 0.05 <= r["E_ref"] <= 2.0, (name, s, r["E_ref"])
            lo, hi = min(lo, r["E_ref"]), max(hi, r["E_ref"])
        else:
            assert r["E_ref"] == 0.0
        assert (r["scale_E"] > 0).tolist() == [bool(m) and bool(v) for m, v in zip(r["members"], r["scale_E"] > 0)]
    print(f"E_ref {lo:.3f} .. {hi:.3f}; the restatement's energies / scale_E at most {worst_e}")


def test_conditioning_terms_by_hand():
    """Two atoms, one pair: S and K are the table's entries, written out."""
    T = rr.tables([0.68, 0.68], [[0, 1]], np.zeros((0, 4)))
    x0 = np.array([[0.0, 0, 0], [1.5, 0, 0]])
    x = np.array([[0.0, 0, 0], [1.7, 0, 0]])
    c = rr.conditioning(x, x0, T)
    d, d0 = np.sqrt(1.7 ** 2 + 1e-7), np.sqrt(1.5 ** 2 + 1e-7)
    assert np.allclose(c["S"], 200 * (d - d0), rtol=1e-14) and np.allclose(c["K"], 200 * (d + d0), rtol=1e-14)
    assert np.isclose(c["scale_E"][0], 2.0 ** -24 * (100 * (d - d0) ** 2 + 200 * (d - d0) * (d + d0)), rtol=1e-14)
    assert c["members"].tolist() == [1, 0, 0] and not c["contact"].any() and not c["scale_E"][1:].any()
    # three atoms far from bonded, 1 A apart where sigma is 2.176: a contact
    T = rr.tables([0.68] * 2, np.zeros((0, 2)), np.zeros((0, 4)))
    c = rr.conditioning(np.array([[0.0, 0, 0], [1.0, 0, 0]]), x0, T)
    sig, d = 1.36 * 1.6, np.sqrt(1 + 1e-7)
    assert np.allclose(c["S"], 60 * (sig - d)) and np.allclose(c["K"], 60 * (d + sig)) and c["contact"].all()
    assert np.isclose(c["scale_E"][2], 2.0 ** -24 * (30 * (sig - d) ** 2 + 60 * (sig - d) * (d + sig)))
    # a weight override changes the torsion term of energy() and nothing else
    w = rc.get("weight_threshold")
    e_own = rr.energy(w["xyz"][2], w["xyz0"][2], w["T"])[0]
    e_off = rr.energy(w["xyz"][2], w["xyz0"][2], w["T"], w=np.zeros(4, dtype=bool))[0]
    assert e_off[1] == 0.0 and e_own[1] > 0 and e_off[0] == e_own[0] and e_off[2] == e_own[2]


def test_tiny():
    c = rc.get("tiny_n1")
    assert len(c["T"]["pairs"]) == 0 and len(c["quads"]) == 0 and len(c["T"]["free_i"]) == 0
    for refs in c["refs"]:
        assert not refs[0]["e"].any() and not refs[0]["g"].any() and not refs[0]["scale"].any() and not refs[0]["members"].any()
    for name, n, n_fixed in (("tiny_n2", 2, 0), ("tiny_n3", 3, 0), ("tiny_n2_fixed0", 2, 1)):
        c = rc.get(name)
        assert c["xyz"].shape == (3, n, 3) and c["fixed"].sum() == n_fixed and c["fixed"][1:].sum() == 0
        for refs in c["refs"]:
            assert refs[0]["members"].tolist() == [n * (n - 1) // 2, 0, 0] and refs[0]["e"][0] > 0
            assert np.abs(refs[0]["g"][~c["fixed"]]).max(-1).min() > 1.0          # every free atom has a gradient to compare


def test_start():
    c = rc.get("start")
    base = tr.case(257)
    assert np.array_equal(c["xyz"], base["xyz0"]) and np.array_equal(c["xyz0"], base["xyz0"])
    for s, refs in enumerate(c["refs"]):
        r = refs[0]
        assert np.abs(rc.sigma_gap(c["xyz"][s], c["T"])).min() >= rc.MARGIN, s
        assert r["e"][0] == 0.0 and r["e"][1] == 0.0 and r["e"][2] > 0 and not r["scale_E"][:2].any()
        assert not r["g"][~r["contact"]].any() and not r["S"][~r["contact"]].any()
        assert 10 < r["contact"].sum() < 257 and (~r["fixed"] & r["contact"]).sum() > 10


def test_far_is_the_same_structure_to_float64():
    base, xyz0, xyz = rc.far_base()
    c = rc.get("far")
    assert np.abs(c["xyz"]).max() < 2048
    for a, b in ((xyz0, c["xyz0"]), (xyz, c["xyz"])):
        assert np.array_equal(b.astype(np.float64), a.astype(np.float64) + rc.FAR_SHIFT)             # the translation is exact
    assert np.abs(xyz - base["xyz"]).max() <= rc.FAR_GRID * 200 and np.abs(xyz0 - base["xyz0"]).max() <= rc.FAR_GRID / 2
    shift = rc.FAR_SHIFT.astype(F32)
    worst = 0.0
    for s in range(3):
        r = c["refs"][s][0]
        e_here = rr.energy(xyz[s], xyz0[s], c["T"], c["fixed"])[0]
        assert (np.abs(r["e"] - e_here) <= r["scale_E"]).all(), s
        assert np.abs(rc.sigma_gap(c["xyz"][s], c["T"])).min() >= rc.MARGIN
        sines = rr.angle_sines(c["xyz0"][s].astype(np.float64), c["quads"])
        assert not ((sines >= 0.05) & (sines <= 0.2)).any()
        assert (r["members"] > 0).all()
        # the same translation of case(257) as it is: rounded, it is another structure
        e_raw = rr.energy(base["xyz"][s] + shift, base["xyz0"][s] + shift, c["T"], c["fixed"])[0]
        raw = np.abs(e_raw - base["ref64"][s][0]) / rr.conditioning(base["xyz"][s], base["xyz0"][s], c["T"])["scale_E"]
        assert raw.min() > 1.0
        worst = max(worst, float(raw.max()))
    print(f"case(257) translated without the grid: energies up to {worst:.0f} scale_E off")


def test_coincident():
    c = rc.get("coincident")
    T = c["T"]
    free = {(int(i), int(j)) for i, j in zip(T["free_i"], T["free_j"])}
    sig, kc = 2 * T["radius"][0] * rr.DEFAULTS["contact_scale"], rr.DEFAULTS["k_c"]         # the float32 radius, as given
    for s in range(3):
        x = c["xyz"][s].astype(np.float64)
        planted = np.zeros(len(T["free_i"]), dtype=bool)
        for a, b, delta in rc.COINCIDENT_PAIRS:
            assert (a, b) in free
            d = np.linalg.norm(x[a] - x[b])
            assert d == 0.0 if delta == 0 else abs(d / delta - 1) < 0.02, (s, a, b, d)
            planted |= (T["free_i"] == a) & (T["free_j"] == b)
        assert np.abs(rc.sigma_gap(x, T))[~planted].min() >= rc.MARGIN
        # the repulsion energy pair by pair; the pair at distance 0 counts k_c (sigma - sqrt(1e-7))^2 and pushes nothing
        d = np.sqrt(((x[T["free_i"]] - x[T["free_j"]]) ** 2).sum(-1) + 1e-7)
        terms = np.where(d < sig, kc * (sig - d) ** 2, 0.0)
        r = c["refs"][s][0]
        assert np.isclose(terms.sum(), r["e"][2], rtol=1e-12)
        zero = (T["free_i"] == 4) & (T["free_j"] == 20)
        assert np.isclose(terms[zero][0], kc * (sig - np.sqrt(1e-7)) ** 2, rtol=1e-12)
        assert not (x[4] - x[20]).any()                           # its force is coefficient x (x_a - x_b) = 0


def test_many_quads():
    bonds, paths = rc.many_graph()
    assert len(bonds) == 99 and len(paths) == 558 and len({tuple(p) for p in paths}) == 558
    adj = {(int(i), int(j)) for i, j in bonds} | {(int(j), int(i)) for i, j in bonds}
    assert all((a, b) in adj and (b, c) in adj and (c, d) in adj and len({a, b, c, d}) == 4 for a, b, c, d in paths.tolist())
    assert paths.tolist() == sorted(paths.tolist(), key=lambda p: (p[1], p[2], p[0], p[3]))
    for count in rc.MANY_COUNTS:
        c = rc.get(f"many_quads_{count}")
        assert len(c["quads"]) == count and len(c["radius"]) == 100 and np.array_equal(c["quads"], paths[:count])
        assert np.array_equal(c["xyz"], rc.get("many_quads_0")["xyz"])
        for s in range(3):
            assert c["refs"][s][0]["members"][1] == count
            if count:
                for dt in (np.float64, F32):
                    assert rr.start_constants(c["xyz0"][s], c["T"], dt)[3].all()
                assert rr.angle_sines(c["xyz0"][s].astype(np.float64), c["quads"]).min() >= 0.2
    # one row block of 256 threads: 513 rows need a third pass, and rows q with q % 256 >= 100 belong to a thread with no atom
    assert 513 > 2 * 256 and 255 % 256 >= 100 and 100 < 256


def test_weight_threshold():
    c = rc.get("weight_threshold")
    T = c["T"]
    assert [u is not None for u in c["undecided"]].count(True) == 2
    for s in range(3):
        s64 = rr.angle_sines(c["xyz0"][s].astype(np.float64), c["quads"])
        w64, w32 = rr.start_constants(c["xyz0"][s], T)[3], rr.start_constants(c["xyz0"][s], T, F32)[3]
        assert (s64[:, 1] > 0.5).all()                                       # the first bond angle is the flatter one
        undecided = []
        for q, target in enumerate(rc.WT_TARGETS[s]):
            gap = s64[q, 0] - 0.1
            if isinstance(target, str):
                assert abs(gap) <= 2 * rc.ULP_01 and (gap >= 0) == (target == "hi"), (s, q, gap)
                undecided.append(q)
                continue
            assert abs(gap) > 8 * 2.0 ** -24 and w64[q] == w32[q] == (gap > 0), (s, q, gap)     # decided
            if target is not None:
                assert abs(s64[q, 0] / target - 1) < 2.0 ** -14 and bool(w64[q]) == (target == rc.WT_ABOVE), (s, q)
        assert len(undecided) <= 1 and undecided == ([] if c["undecided"][s] is None else [c["undecided"][s]])
        refs = c["refs"][s]
        assert len(refs) == 1 + len(undecided)
        if undecided:
            assert [bool(r["members"][1] == w64.sum() - w64[undecided[0]] + v) for r, v in zip(refs, (0, 1))] == [True, True]
        # the restatement with its OWN weights keeps rule 1 against one of the references
        e32, g32, _ = rr.energy(c["xyz"][s], c["xyz0"][s], T, dtype=F32)
        assert rc.passes(rc.judge_any(refs, e32, g32)), s
    # the two undecided structures fall on different sides in float64; on one of them the restatement disagrees with float64
    sides = [bool(rr.start_constants(c["xyz0"][s], T)[3][2]) for s in (0, 1)]
    sides32 = [bool(rr.start_constants(c["xyz0"][s], T, F32)[3][2]) for s in (0, 1)]
    assert sides == [True, False] and sides32 != sides


def test_batch():
    c = rc.get("batch")
    assert c["xyz"].shape == (130, 40, 3) and rc.BATCH_SIZES == (64, 65, 130) and max(rc.BATCH_PLANTED) == 129
    assert all(s in rc.BATCH_PLANTED for s in (0, 63, 64, 129))                  # the structures compared alone are not idle
    for s in range(130):
        under = int((rc.sigma_gap(c["xyz_loop"][s], c["T"]) < 0).sum())
        assert (under > 0) == (s in rc.BATCH_PLANTED), s
    for s in (0, 1, 64, 66):
        out = rr.minimise(c["xyz_loop"][s], c["T"], rc.BATCH_ITER)
        assert bool(out["converged"]) == (s not in rc.BATCH_PLANTED)
        assert out["accepted"].any() == (s in rc.BATCH_PLANTED)


def test_loop_runs_reject_and_decide_clearly():
    """The float64 loop over the first K trials: the second run rejects at least 3 on a structure at the chosen step (and
    does not at 0.1), and no decision of either run is close - the smallest |E' - E| / E against bounds of about 1e-7."""
    runs = rc.loop_runs()
    rejected = {}
    for name, r in runs.items():
        for s in range(len(r["xyz"])):
            out = rr.minimise(r["xyz"][s], r["T"], rc.LOOP_K, r["fixed"], **r["constants"])
            e, et = out["energy"][:-1], out["trial_energy"]
            margin = float((np.abs(et - e) / e).min())
            ref = rc.structure_ref(r["xyz"][s], r["xyz"][s], r["T"], r["fixed"])
            bound = rc.FACTOR * ref["scale_E"].sum() / e[0]
            rejected[name, s] = int((~out["accepted"]).sum())
            print(f"{name}[{s}]: {rejected[name, s]} of {rc.LOOP_K} rejected, smallest margin {margin:.1e}, bound {bound:.1e}")
            assert margin > 1e-4 and 2 * bound < 1e-5
    assert max(rejected["c257", s] for s in range(3)) >= 3
    r = runs["c257"]
    at_01 = [int((~rr.minimise(r["xyz"][s], r["T"], rc.LOOP_K, r["fixed"], h0=0.1, h_max=0.1)["accepted"]).sum()) for s in range(3)]
    assert max(at_01) < 3 and rc.LOOP_H == 0.2
