"""CPU checks of the secondary-structure assignment: the C ABI declares and exports the two entry points and rejects bad
arguments before any HIP call, the kernels use no scratch, metrics.dssp_tables is right, the reference of
tests/dssp_ref.py gives the hand-derived labels on every planted case, and the planted cases keep the margins that the GPU
tests (tests/test_dssp.py) rely on.

Figures of the reference (printed by every run): the float32 restatement deviates from float64 by at most 3.8e-5 kcal/mol
in an eligible energy, 2.4e-2 degrees in kappa (at kappa = 0.01 degrees, where acos is ill-conditioned; 1e-5 near 70) and
1.0e-7 A in a link distance; the smallest |E + 0.5| of a planted case is 0.0039 kcal/mol, the smallest |kappa - 70| 0.48
degrees, the smallest | |C-N| - 2.5 | 0.5 A; no pair of the noisy copies (104 k eligible pairs) is undecided."""
import argparse
import json
import os
import re

import numpy as np
import pytest
import torch

from codlad_amd import _lib, build, metrics
from tests import dssp_ref as dr
from tests.cli_script import load_cli

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("codlad_dssp_hbonds", "codlad_dssp_assign")
E_MARGIN, KAPPA_MARGIN, LINK_MARGIN = 1e-3, 0.01, 1e-3          # kcal/mol, degrees, A: what a planted case keeps
UNDECIDED_CAP = 1e-4                                            # of the eligible pairs of the noisy copies


def all_planted():
    cases = {name: (top, x) for name, (top, x, _want) in dr.planted().items()}
    cases.update({f"sized_{R}": dr.sized(R) for R in dr.SIZES})
    return cases


def test_header_exports_signatures_and_abi_agree():
    header = open(os.path.join(ROOT, "include", "codlad_hip.h")).read()
    lib = _lib.lib()
    for name in ENTRY_POINTS:
        decl = re.findall(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
        assert len(decl) == 1, name
        assert len(decl[0].split(",")) == len(_lib._SIGS[name][1]), name               # one ctypes entry per parameter
        assert name in _lib.exported_symbols() and hasattr(lib, name), name
        assert not name.startswith(("codlad_ens_", "codlad_stereo_"))
    assert "#define CODLAD_ABI_VERSION 19\n" in header and lib.codlad_abi_version() == 19 == _lib.ABI_VERSION
    assert f"#define CODLAD_DSSP_MAX_RES {_lib.DSSP_MAX_RES}\n" in header and _lib.DSSP_MAX_RES >= 4096
    names = ("LOOP", "H", "B", "E", "G", "I", "T", "S")
    for code, name in enumerate(names):
        assert f"#define CODLAD_DSSP_{name} {code}\n" in header, name
    assert _lib.DSSP_CODES == " HBEGITS" == dr.CODES and metrics.DSSP_CODES == _lib.DSSP_CODES
    for name, value in (("KIND_PRO", _lib.DSSP_KIND_PRO), ("KIND_CHAIN_START", _lib.DSSP_KIND_CHAIN_START),
                        ("GEOM_LINK", _lib.DSSP_GEOM_LINK), ("GEOM_BEND", _lib.DSSP_GEOM_BEND),
                        ("UNDEFINED", _lib.DSSP_UNDEFINED)):
        assert f"#define CODLAD_DSSP_{name} {value}\n" in header, name
    assert (dr.KIND_PRO, dr.KIND_CHAIN_START, dr.GEOM_LINK, dr.GEOM_BEND, dr.UNDEFINED) == (1, 2, 1, 2, 255)
    # every new define carries the one prefix
    new = header[header.index("Secondary structure (csrc/dssp_kernels.hip)"):header.index("Self-test of the MFMA chain")]
    assert all(d.startswith("CODLAD_DSSP_") for d in re.findall(r"#define (\w+)", new))


def test_source_is_built_without_contraction_and_without_scratch():
    assert "dssp_kernels.hip" in build.SOURCES and build.EXTRA_FLAGS["dssp_kernels.hip"] == ["-ffp-contract=off"]
    build.build(force=False, verbose=False)
    if not os.path.exists(build.RESOURCES):
        build.build(force=True, verbose=False)
    with open(build.RESOURCES) as f:
        table = json.load(f)
    mine = {k: v for k, v in table.items() if v.get("source") == "dssp_kernels.hip"}
    for kernel in ("dssp_prep_kernel", "dssp_hbond_kernel", "dssp_assign_kernel"):
        assert sum(kernel in k for k in mine) == 1, sorted(mine)
    for name, r in mine.items():
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0, (name, r)
        if "dssp_hbond_kernel" in name:
            assert r["VGPRs"] <= 128, (name, r)                                       # four waves per SIMD or more


def test_argument_errors_return_a_negative_code_before_any_hip_call():
    """No GPU here: a call that got as far as a launch would return a positive hipError_t (or crash)."""
    lib = _lib.lib()
    buf = np.zeros(64, dtype=np.float64)                 # any non-null, 16-byte aligned host address: never dereferenced
    p = buf.ctypes.data
    assert p % 16 == 0
    ok = [p, 1, 40, p, p, 10, p, p, p, p, p, p, p, None]
    cases = [(k, None) for k in (0, 3, 4, 6, 7, 8, 9, 10, 11, 12)]
    cases += [(1, 0), (1, -1), (2, 0), (2, -3), (5, 0), (5, -1), (5, _lib.DSSP_MAX_RES + 1), (3, p + 4), (3, p + 8)]
    for k, bad in cases:
        args = list(ok)
        args[k] = bad
        assert lib.codlad_dssp_hbonds(*args) < 0, (k, bad)
        assert b"codlad_dssp_hbonds" in lib.codlad_last_error(), (k, bad)
    assert lib.codlad_dssp_hbonds(p, 2 ** 30, 40, p, p, 10, p, p, p, p, p, p, p, None) < 0           # the launch-grid bound
    assert b"workgroups" in lib.codlad_last_error()
    assert lib.codlad_dssp_hbonds(p, 1, 2 ** 30, p, p, 10, p, p, p, p, p, p, p, None) < 0
    oka = [p, p, p, p, 1, 10, p, p, p, None]
    cases = [(k, None) for k in (0, 1, 2, 3, 6, 7, 8)] + [(4, 0), (4, -1), (5, 0), (5, -2), (5, _lib.DSSP_MAX_RES + 1)]
    for k, bad in cases:
        args = list(oka)
        args[k] = bad
        assert lib.codlad_dssp_assign(*args) < 0, (k, bad)
        assert b"codlad_dssp_assign" in lib.codlad_last_error(), (k, bad)
    assert lib.codlad_dssp_assign(p, p, p, p, 2 ** 20, 4096, p, p, p, None) < 0
    assert b"too many residues" in lib.codlad_last_error()


def test_dssp_tables_on_built_topologies():
    for name, (top, _x) in all_planted().items():
        bb, kind = metrics.dssp_tables(top)
        want_bb, want_kind = dr.tables(top)
        assert bb.dtype == torch.int32 and tuple(bb.shape) == (top.n_residues, 4) and kind.dtype == torch.uint8, name
        assert np.array_equal(bb.numpy(), want_bb) and np.array_equal(kind.numpy(), want_kind), name
        assert metrics.dssp_tables(top)[0] is bb                                    # built once, kept on the topology
        for r in range(top.n_residues):                                             # by name, not by position
            got = [top.name[a] if a >= 0 else None for a in bb[r].tolist()]
            assert got == [a if a in top.atom_names[r] else None for a in ("N", "CA", "C", "O")], (name, r)
    top = dr.planted()["helix_no_o"][0]
    assert metrics.dssp_tables(top)[0][5].tolist()[3] == -1 and (metrics.dssp_tables(top)[0][:, :3] >= 0).all()
    kind = metrics.dssp_tables(dr.planted()["helix_pro"][0])[1].tolist()
    assert kind == [2] + [0] * 6 + [1] + [0] * 6
    assert metrics.dssp_tables(dr.planted()["helix_chain_start"][0])[1].tolist() == [2] + [0] * 6 + [2] + [0] * 6
    assert metrics.dssp_tables(dr.planted()["sheet_anti"][0])[1].tolist() == [2] + [0] * 6 + [2] + [0] * 6


def test_reference_gives_the_hand_derived_labels_on_every_planted_case():
    for name, (top, x, want) in dr.planted().items():
        r = dr.reference(x, top)
        assert r["ss_string"] == [want], (name, r["ss_string"])
        assert r["counts"][0].tolist() == [want.count(c) for c in dr.CODES], name
    # the bonds behind the labels: 4-, 3- and 5-turns only in the three helices
    for kind, n in (("alpha", 4), ("310", 3), ("pi", 5)):
        top, x, _w = dr.planted()["helix_" + kind]
        hb = dr.reference(x, top)["hb"][0]
        assert sorted(zip(*np.nonzero(hb))) == [(i, i + n) for i in range(14 - n)], kind
    for kind in ("anti", "par"):
        top, x, _w = dr.planted()["sheet_" + kind]
        r = dr.reference(x, top)
        between = {(int(i), int(j)) for i, j in zip(*np.nonzero(r["hb"][0])) if (i < 7) != (j < 7)}
        assert between == set(dr.DOCK_BONDS[kind]), kind
        col = 1 if kind == "anti" else 0
        partners = r["bridge"][0, 1:6, col].tolist()
        assert partners == ([12, 11, 10, 9, 8] if kind == "anti" else [8, 9, 10, 11, 12]) and (r["bridge"][0, :, 1 - col] == -1).all()
    # what each of the remaining cases plants is in the bonds and the links
    r = dr.reference(*dr.planted()["helix_break_helix"][1::-1])
    assert not r["link"][0, 14] and r["link"][0, :14].all() and r["link"][0, 15:29].all()
    assert abs(r["d_link"][0, 14] - 3.0) < 1e-5 and not r["eligible"][0, :, 15].any()
    r = dr.reference(*dr.planted()["helix_pro"][1::-1])
    assert not r["eligible"][0, :, 7].any() and not r["hb"][0, 3, 7] and r["hb"][0, 2, 6] and r["hb"][0, 4, 8]
    r = dr.reference(*dr.planted()["helix_chain_start"][1::-1])
    assert not r["link"][0, 6] and abs(r["d_link"][0, 5] - 1.329) < 1e-5 and np.isnan(r["d_link"][0, 6])
    assert not r["eligible"][0, :, 7].any() and r["hb"][0, 4, 8]
    r = dr.reference(*dr.planted()["helix_no_o"][1::-1])
    assert not r["eligible"][0, 5].any() and not r["eligible"][0, :, 6].any() and r["link"][0, 5]


def test_hand_written_bitmaps_give_the_hand_derived_labels():
    for R in (130, 200):
        hb, link, bend, checks = dr.handmade(R)
        ss, bridge, counts = dr.assign(hb, link, bend)
        got = dr.labels(ss)
        assert {r: got[r] for r in checks} == checks, R
        assert counts.sum() == R and set(got) == set(dr.CODES)                       # every state occurs
        b_anti, b_par = (64, 128) if R == 130 else (128, 64)
        assert bridge[10:17, 1].tolist() == [b_anti + 2 - k for k in range(7)]      # partners on both sides of the boundary
        assert bridge[20:25, 0].tolist() == [b_par - 4 + k for k in range(5)]
        assert bridge[52].tolist() == [-1, 88] and bridge[50].tolist() == [-1, -1] and bridge[40].tolist() == [-1, -1]
        acc, don = dr.pack_bits(hb)
        assert acc.shape == (R, (R + 63) // 64) and acc.dtype == np.uint64
        assert np.array_equal(dr.unpack_bits(acc, R), hb) and np.array_equal(dr.unpack_bits(don, R), hb.T)
        assert (int(acc[10, (b_anti + 2) // 64]) >> ((b_anti + 2) % 64)) & 1


def test_planted_cases_keep_their_margins():
    """With these margins the float32 stage cannot flip a planted decision: every deviation of the float32 restatement is
    orders of magnitude inside them, and no pair, bend or link of a planted case is undecided."""
    for name, (top, x) in all_planted().items():
        m = dr.margins(x[None], top)
        print(f"{name}: min |E + 0.5| {m['min_e']:.4f}, min |kappa - 70| {m['min_k']:.3f}, min ||C-N| - 2.5| {m['min_d']:.3f}; "
              f"float32 deviation {m['dev_e']:.2e} kcal/mol, {m['dev_k']:.2e} deg, {m['dev_d']:.2e} A")
        assert m["min_e"] >= E_MARGIN and m["min_k"] >= KAPPA_MARGIN and m["min_d"] >= LINK_MARGIN, name
        assert 4.0 * m["dev_e"] < E_MARGIN and 4.0 * m["dev_d"] < LINK_MARGIN, name
        assert not m["undecided_e"].any() and not m["undecided_k"].any() and not m["undecided_d"].any(), name
        # the restatement itself takes every decision as float64 does
        for key in ("hb", "link", "bend", "eligible"):
            assert np.array_equal(m["r64"][key], m["r32"][key]), (name, key)
    assert dr.margins(dr.planted()["sheet_par"][1][None], dr.planted()["sheet_par"][0])["min_e"] >= 0.04


def test_noisy_copies_stay_within_the_cap_of_undecided_pairs():
    eligible = undecided = 0
    for R in dr.SIZES:
        top, x = dr.sized(R)
        m = dr.margins(dr.noisy(x, 7 * R), top)
        eligible += int(m["r64"]["eligible"].sum())
        undecided += int(m["undecided_e"].sum())
        flips = m["r64"]["hb"] != m["r32"]["hb"]
        assert not (flips & ~m["undecided_e"]).any(), R
        assert m["r64"]["hb"].sum() > 0 or R == 5
    print(f"noisy copies: {undecided} undecided of {eligible} eligible pairs")
    assert eligible > 1e5 and undecided <= UNDECIDED_CAP * eligible


def test_python_layer_rejects_what_it_cannot_run():
    top, x, _w = dr.planted()["helix_alpha"]
    xt = torch.from_numpy(x)[None]
    for call in (lambda: metrics.hbonds(xt, top), lambda: metrics.dssp(xt, top),
                 lambda: metrics.ss_propensity(torch.zeros(2, 3, dtype=torch.uint8))):
        with pytest.raises(RuntimeError, match="CUDA tensor"):
            call()
    assert metrics.DSSP_MAX_RES == _lib.DSSP_MAX_RES and len(metrics.DSSP_NAMES) == 8
    assert metrics.ss_strings(torch.tensor([[0, 1, 2, 3], [4, 5, 6, 7], [255, 255, 255, 255]], dtype=torch.uint8)) == \
        [" HBE", "GITS", "????"]


def test_cli_allows_dssp_exactly_where_the_geometry_check_is_allowed():
    cli = load_cli("codlad_cli")

    def args(**kw):
        base = dict(dssp=True, experiment="latent", data_process=False, synthetic=True, cg_pdb=None)
        base.update(kw)
        return argparse.Namespace(**base)

    a = args(dssp=False)
    assert cli.check_dssp(a) is False and a.dssp is False
    a = argparse.Namespace(experiment="latent", data_process=False, synthetic=True, cg_pdb=None)
    assert cli.check_dssp(a) is False and a.dssp is False                            # an old namespace without the flag
    assert cli.check_dssp(args()) is True and cli.check_dssp(args(experiment="recon")) is True
    for exp in ("bpd", "fmloss"):
        with pytest.raises(SystemExit, match="generates none"):
            cli.check_dssp(args(experiment=exp))
    with pytest.raises(SystemExit, match="topology"):
        cli.check_dssp(args(data_process=True, synthetic=False))
    assert cli.check_dssp(args(cg_pdb=["x.pdb"], synthetic=False)) is True
