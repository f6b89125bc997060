"""CPU checks of the pair-histogram feature: the C ABI of codlad_pair_hist and codlad_pair_hist_profile (declared,
exported, bad arguments refused before any HIP call), what the Python layer refuses, and the references of
tests/pair_hist_ref.py against each other - the float32 restatement of the bin decision against the float64 histogram by the
sandwich, and the derived bounds of the histogram profile and of the second moment for the float64 reference alone.

delta of a case is 4 x the largest |t32 - t64| of its pairs (t = r / dr in bins): the restatement's own deviation, nothing
of the device's output; test_inputs_keep_their_pairs_off_the_bin_edges holds the cases to it and prints it."""
import argparse
import importlib
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

from codlad_amd import _lib, build, metrics
from codlad_amd.utils.cg_input import template_topology
from tests import pair_hist_ref as pr
from tests import saxs_ref as sr
from tests.cli_script import load_cli

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pd = importlib.import_module("codlad_amd.metrics.pair_distribution")      # metrics.pair_distribution is the function


def test_header_declares_and_library_exports_both_entry_points():
    header = open(os.path.join(ROOT, "include", "codlad_hip.h")).read()
    lib = _lib.lib()
    for name, n_args in (("codlad_pair_hist", 15), ("codlad_pair_hist_profile", 22)):
        decl = re.findall(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", header)
        assert len(decl) == 1, name
        assert name in _lib.exported_symbols() and hasattr(lib, name)
        assert len(_lib._SIGS[name][1]) == decl[0].count(",") + 1 == n_args, name
    for macro, value in (("MAX_BINS", 4096), ("MAX_ATOMS", 65535), ("ITEM_WORDS", 5), ("ROWS", 64)):
        assert f"#define CODLAD_PAIR_HIST_{macro} {value}" in header and getattr(_lib, f"PAIR_HIST_{macro}") == value
    assert (pr.MAX_BINS, pr.MAX_ATOMS) == (metrics.PAIR_HIST_MAX_BINS, metrics.PAIR_HIST_MAX_ATOMS) == (4096, 65535)
    assert "#define CODLAD_PAIR_HIST_CLASS(a, b, T) ((a) * (T) - (a) * ((a) - 1) / 2 + ((b) - (a)))" in header
    assert "pair_hist_kernels.hip" in build.SOURCES and build.EXTRA_FLAGS["pair_hist_kernels.hip"] == ["-ffp-contract=off"]


def test_pair_hist_kernels_use_no_scratch():
    import json
    build.build(force=False, verbose=False)
    if not os.path.exists(build.RESOURCES):
        build.build(force=True, verbose=False)
    with open(build.RESOURCES) as f:
        table = json.load(f)
    mine = {k: v for k, v in table.items() if v.get("source") == "pair_hist_kernels.hip"}
    assert any("pair_hist_kernel" in k for k in mine) and any("profile_class_kernel" in k for k in mine), sorted(mine)
    for name, r in mine.items():
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0, (name, r)


def test_argument_errors_return_a_negative_code_before_any_hip_call():
    """No GPU here: a call that got as far as a launch would return a positive hipError_t (or crash)."""
    lib = _lib.lib()
    buf = np.zeros(64, dtype=np.float64)                 # any non-null host address: never dereferenced by these calls
    p = buf.ctypes.data
    #     xyz S  n  order start T  inv_dr B  items n_items H  over d_bin finite stream
    ok = [p, 1, 4, p, p, 2, 2.0, 8, p, 1, p, p, p, p, None]
    cases = [(k, None) for k in (0, 3, 4, 8, 10, 11, 12, 13)]
    cases += [(1, 0), (1, -1), (2, 0), (2, -3), (9, 0), (9, -1), (7, 0), (7, -1), (7, 4097), (2, 65536), (5, 0), (5, -1), (5, 33),
              (6, 0.0), (6, -1.0), (6, float("nan")), (6, float("inf")), (1, 2 ** 31 - 1)]
    for k, bad in cases:
        args = list(ok)
        args[k] = bad
        if (k, bad) == (1, 2 ** 31 - 1):
            args[9] = 2                                  # two items a structure: the grid passes 2^31
        assert lib.codlad_pair_hist(*args) < 0, (k, bad)
        assert b"codlad_pair_hist" in lib.codlad_last_error(), (k, bad)
    args = list(ok)
    args[2], args[7], args[5] = 65535, 4096, 32          # the caps themselves are inside: nothing to refuse, so no call here
    #     H over d_bin finite S  T  B  count ff sinc Q  partial I  mean_I w  r2 P  I0 m2 mean_P complete stream
    ok = [p, p, p, p, 1, 2, 8, p, p, p, 4, p, p, p, p, p, p, p, p, p, p, None]
    cases = [(k, None) for k in (0, 1, 2, 3, 7, 20)]
    cases += [(8, None), (9, None), (11, None),           # the profile is asked for (I given): its tables must be there
              (14, None), (15, None), (17, None), (18, None),     # so is the pair distribution (P given)
              (4, 0), (4, -1), (6, 0), (6, -1), (6, 4097), (5, 0), (5, 33), (10, 0), (10, -1), (10, 513)]
    for k, bad in cases:
        args = list(ok)
        args[k] = bad
        assert lib.codlad_pair_hist_profile(*args) < 0, (k, bad)
        assert b"codlad_pair_hist_profile" in lib.codlad_last_error(), (k, bad)
    for drop in ((12, 16), (12,), (16,)):                # neither I nor P; a mean without its rows
        args = list(ok)
        for k in drop:
            args[k] = None
        assert lib.codlad_pair_hist_profile(*args) < 0, drop


def test_python_layer_refuses_what_it_cannot_run():
    top = template_topology(["ALA", "GLY", "SER"])
    x = torch.zeros(2, top.n_atoms, 3)
    for call in (lambda: metrics.pair_histogram(x, top), lambda: metrics.pair_distribution(x, top),
                 lambda: metrics.saxs_profile_hist(x, top), lambda: metrics.pair_histogram_lists(x, [0] * top.n_atoms, 1)):
        with pytest.raises(RuntimeError, match="CUDA tensor"):
            call()
    assert not [k for k in top.__dict__ if "pair" in k or "hist" in k]              # refused before any table was built
    tables = lambda t, T, dr=0.5, r_max=20.0: pd._hist_tables(t, T, dr, r_max, "cpu")        # noqa: E731
    t = tables([1, 0, 1, 1], 3)
    assert t["order"].tolist() == [1, 0, 2, 3] and t["type_start"].tolist() == [0, 1, 4, 4] and t["count"].tolist() == [1, 3, 0]
    assert (t["order"].dtype, t["items"].dtype, t["n_bins"], t["inv_dr"]) == (torch.int32, torch.int32, 40, 2.0)
    assert t["edges"].tolist() == [0.5 * b for b in range(41)] and t["classes"].tolist() == [list(c) for c in pr.classes(3)]
    for bad_dr in (0, -0.5, float("nan"), float("inf"), "wide", None):
        with pytest.raises(ValueError, match="dr and r_max"):
            tables([0], 1, dr=bad_dr)
    for bad_r in (0, -3.0, float("nan"), "far"):
        with pytest.raises(ValueError, match="dr and r_max"):
            tables([0], 1, r_max=bad_r)
    assert tables([0], 1, 0.5, 2048.0)["n_bins"] == 4096
    with pytest.raises(ValueError, match="at most 4096 bins"):
        tables([0], 1, 0.5, 2048.5)
    with pytest.raises(ValueError, match="at most 4096 bins"):
        metrics.pair_histogram(_FakeCuda(x), top, dr=0.01, r_max=100.0)
    with pytest.raises(ValueError, match="at most 65535 atoms"):
        tables(np.zeros(65536, dtype=np.int64), 1)
    for bad_types, T in (([0, 2], 2), ([-1, 0], 2), ([], 1)):
        with pytest.raises(ValueError, match="atom type"):
            tables(bad_types, T)
    for T in (0, 33):
        with pytest.raises(ValueError, match="atom types"):
            tables([0], T)
    limit = metrics.SAXS_Q_LIMIT
    for bad_q in ([np.nan], [-0.1], [limit * 1.001], [np.inf]):
        with pytest.raises(ValueError, match="every q"):
            pd._check_q("saxs_profile_hist", bad_q)
    with pytest.raises(ValueError, match="q values"):
        pd._check_q("saxs_profile_hist", np.linspace(0, 0.5, 513))
    assert pd._check_q("saxs_profile_hist", None).shape == (51,)
    with pytest.raises(ValueError, match="every q"):
        metrics.saxs_profile_hist(_FakeCuda(x), top, q=[0.1, -1.0])
    with pytest.raises(ValueError, match="result of pair_histogram"):
        metrics.saxs_profile_hist(None, top, hist={"H": x})
    assert not [k for k in top.__dict__ if "pair" in k or "hist" in k]


class _FakeCuda:
    """What the refusals that precede every launch read of xyz: is_cuda and device (nothing here reaches a launch)."""
    is_cuda, device = True, "cuda"

    def __init__(self, t):
        self.t = t


def test_work_items_cover_every_pair_once():
    for counts, cols in (([1], 8), ([5, 0, 1, 130], 64), ([64, 65, 63], 100), ([200], 64), ([3, 300], 2048)):
        start = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
        items = pd._work_items(start, cols)
        assert items.dtype == np.int32 and items.shape[1] == 5 and items.shape[0] >= 1
        n = int(start[-1])
        seen = np.zeros((n, n), dtype=np.int64)
        for a, b, row0, c0, c1 in items.tolist():
            assert a <= b and c0 <= c1 <= start[b + 1] and (c1 - c0) <= cols
            if c1 > c0:
                assert start[a] <= row0 < start[a + 1] and start[b] <= c0
            rows = np.arange(row0, min(row0 + 64, start[a + 1]))
            for j in range(c0, c1):
                seen[rows[(rows < j) | (a != b)], j] += 1
        assert np.array_equal(seen, np.triu(np.ones((n, n), dtype=np.int64), 1)), counts


def test_class_index_round_trips():
    for T in (1, 5, 32):
        rows = metrics.pair_classes(T)
        assert rows.shape == (T * (T + 1) // 2, 2) and rows.tolist() == [list(c) for c in pr.classes(T)]
        for c, (a, b) in enumerate(rows.tolist()):
            assert a <= b and metrics.pair_class_index(a, b, T) == c == pr.class_index(a, b, T)
        assert len({tuple(r) for r in rows.tolist()}) == rows.shape[0]


def test_cases_cover_the_sizes_the_issue_names():
    keys = pr.case_keys()
    assert {k[0] for k in keys} == {1, 2, 63, 64, 65, 129, 300}
    assert {k[1] for k in keys} == {1, 5, 32} and {k[2] for k in keys} == {1, 64, 65, 400}
    assert {k[3] for k in keys} == {0.5, 0.1} and {k[4] for k in keys} == {0.0, 500.0}
    for key in keys:
        c = pr.case(key)
        assert c["x"].shape == (3, key[0], 3) and c["x"].dtype == np.float32
        if key[1] >= 3:                                   # a type no atom has and a type with exactly one atom
            assert c["count"][key[1] - 1] == 0 and c["count"][key[1] - 2] == 1
        for arr in c.values():
            if isinstance(arr, np.ndarray):
                assert not arr.flags.writeable
    assert any(pr.case(k)["over32"].any() for k in keys) and any(not pr.case(k)["over32"].any() for k in keys)


def test_inputs_keep_their_pairs_off_the_bin_edges():
    """A condition on the inputs: in every case with 1 000 pairs or more at most 0.1 % of the pairs lie within delta of a
    bin edge under the float64 reference, in every smaller case none does."""
    shown = []
    for key in pr.case_keys():
        c = pr.case(key)
        shown.append(f"{pr.case_id(key)} delta {c['delta']:.2e} near {c['near']:.2e}")
        assert c["near"] <= (1e-3 if c["n_pairs"] >= 1000 else 0.0), (key, c["near"], c["n_pairs"])
    print("; ".join(shown))


def test_float32_restatement_against_the_float64_histogram():
    """For every class and every bin edge b: #64{t < b - delta} <= sum_{bin < b} H32[c] <= #64{t < b + delta}; and the totals
    are the pair counts of the class."""
    differing = 0
    for key in pr.case_keys():
        c = pr.case(key)
        n, T, B = key[0], key[1], key[2]
        for s in range(pr.N_STRUCT):
            assert pr.sandwich(c["H32"][s], c["cls"], c["t64"][s], c["delta"], B) == 0, (key, s)
            assert pr.sandwich(c["H64"][s], c["cls"], c["t64"][s], 0.0, B) == 0, (key, s)
            differing += int(np.abs(c["H32"][s] - c["H64"][s]).sum()) // 2
            for ci, (a, b) in enumerate(pr.classes(T)):
                want = c["count"][a] * c["count"][b] if a < b else c["count"][a] * (c["count"][a] - 1) // 2
                assert c["H32"][s, ci].sum() + c["over32"][s, ci] == want == c["H64"][s, ci].sum() + c["over64"][s, ci]
        assert c["H32"].sum() + c["over32"].sum() == 3 * n * (n - 1) // 2
    print(f"pairs whose float32 bin is not the float64 one: {differing} over all cases")


def test_histogram_profile_of_the_reference_stays_within_the_derived_bound():
    """|I_hist,64[k] - I_debye64[k]| <= 0.43618 q_k (dr / 2 + delta dr) 2 sum_{i<j} |f_i f_j| on the GPU cases' own inputs,
    for every structure without a pair beyond the last bin; and |m2_hist - m2| <= sum |w_i w_j| (r dr + dr^2 / 4) pairwise."""
    worst_i = worst_m = 0.0
    checked = 0
    for key in pr.case_keys():
        c = pr.case(key)
        T, B, dr = key[1], key[2], key[3]
        finite = np.ones(3, dtype=bool)
        I, _mean, complete = pr.profile_ref(c["H64"], c["over64"], c["d64"], finite, c["count"], c["ff"], pr.sinc_table(pr.Q_GRID, B, dr))
        ref, _A = sr.debye64(c["x"], c["types"], c["ff"], pr.Q_GRID)
        bound = pr.profile_bound(c["types"], c["ff"], pr.Q_GRID, dr, c["delta"])
        r2 = ((np.arange(B) + 0.5) * dr) ** 2
        _P, _I0, m2, _mp = pr.pr_ref(c["H64"], c["over64"], c["d64"], finite, c["count"], c["w"], r2)
        mom = pr.moment_ref(c["x"], c["types"], c["w"])
        for s in np.nonzero(complete)[0]:
            checked += 1
            err = np.abs(I[s] - ref[s])
            assert (err <= bound).all(), (key, s, (err / np.maximum(bound, 1e-300)).max())
            m_bound = pr.moment_bound(mom[s, 1], mom[s, 2], dr, 0.0)
            assert abs(m2[s] - mom[s, 0]) <= m_bound, (key, s)
            if key[0] > 1:
                worst_i, worst_m = max(worst_i, float((err / bound).max())), max(worst_m, abs(m2[s] - mom[s, 0]) / m_bound)
        assert np.isnan(I[~complete]).all()
    assert checked >= 3 * len(pr.SIZES)
    print(f"float64 reference: max |I_hist - I_debye| / bound {worst_i:.4f}, max |m2_hist - m2| / bound {worst_m:.4f} over "
          f"{checked} complete structures")


def test_contour_length_default_bounds_the_synthetic_structures():
    from codlad_amd import synth
    for i, L in enumerate((12, 46, 120)):
        prot = synth.make_protein(L, 1000 + i, n_frames=2)
        top = template_topology([synth.IDX2THR[int(z)] for z in prot["z_full"]][1:-1])
        r_max = metrics.contour_r_max(top)
        assert r_max == 3.85 * len(top.res_names) + 30.0
        ca = np.asarray(prot["xyz_full"], dtype=np.float64).reshape(2, L + 2, 3)[:, 1:-1]
        for frame in ca:                                  # the CA trace the structures are decoded from; every atom of a
            extent = np.sqrt(((frame[:, None] - frame[None]) ** 2).sum(-1)).max()       # residue lies within 8 A of its CA
            assert extent + 2 * 8.0 < r_max, (L, extent, r_max)
    two = template_topology(["ALA"] * 5, chain_ids=[0, 0, 0, 1, 1])
    assert metrics.contour_r_max(two) == (3.85 * 3 + 30.0) + (3.85 * 2 + 30.0)


def test_cli_allows_pr_exactly_where_observables_are_allowed():
    cli = load_cli("codlad_cli")

    def args(**kw):
        base = dict(pr=None, experiment="latent", data_process=False, synthetic=True, cg_pdb=None)
        base.update(kw)
        return argparse.Namespace(**base)

    a = args()
    assert cli.check_pr(a) == 0 and a.pr == 0
    assert cli.check_pr(args(pr=0.5)) == 0.5 and cli.check_pr(args(pr=0.25, experiment="recon")) == 0.25
    for bad in (0.0, -0.5, float("nan"), float("inf")):
        with pytest.raises(SystemExit, match="bin width"):
            cli.check_pr(args(pr=bad))
    for exp in ("bpd", "fmloss"):
        with pytest.raises(SystemExit, match="generates none"):
            cli.check_pr(args(pr=0.5, experiment=exp))
        with pytest.raises(SystemExit, match="generates none"):
            cli.check_observables(args(observables=960, experiment=exp))
    with pytest.raises(SystemExit, match="topology"):
        cli.check_pr(args(pr=0.5, data_process=True, synthetic=False))
    assert cli.check_pr(args(pr=0.5, cg_pdb=["x.pdb"], synthetic=False)) == 0.5
