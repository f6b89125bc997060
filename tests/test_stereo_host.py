"""CPU checks of the stereochemistry check: the C ABI declares and exports the entry point and rejects bad arguments
before any HIP call, `metrics.stereo_tables` lists the right atoms for every residue template and chain end, the CLI
refuses --stereo_check where it refuses --geometry_check, and the reference the GPU tests compare with
(tests/stereo_ref.py) returns the angles, inversions and peptide-bond classes its builder planted."""
import os
import re
import types

import numpy as np
import pytest
import torch

from codlad_amd import _lib, metrics
from codlad_amd.utils.cg_input import template_topology
from tests import stereo_ref as sr
from tests.cli_script import load_cli

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def cli_module():
    return load_cli("codlad_cli_stereo")


def test_header_declares_and_library_exports_the_entry_point():
    header = open(os.path.join(ROOT, "include", "codlad_hip.h")).read()
    assert re.findall(r"\bint\s+(codlad_stereo_[a-z0-9_]+)\s*\(", header) == ["codlad_stereo_check"]
    lib = _lib.lib()
    assert "codlad_stereo_check" in _lib.exported_symbols() and hasattr(lib, "codlad_stereo_check")
    assert "#define CODLAD_ABI_VERSION 19\n" in header and lib.codlad_abi_version() == 19 == _lib.ABI_VERSION
    for name, bit in dict(_lib.STEREO_FLAGS, columns=_lib.STEREO_COLUMNS, counts=_lib.STEREO_N_COUNTS).items():
        assert f"#define CODLAD_STEREO_{name.upper()} {bit}\n" in header, name
    assert metrics.STEREO_COUNTS == sr.COUNTS and metrics.STEREO_COLUMNS[:3] == ("phi", "psi", "omega")
    assert len(metrics.STEREO_COUNTS) == _lib.STEREO_N_COUNTS and len(metrics.STEREO_COLUMNS) == _lib.STEREO_COLUMNS


def test_argument_errors_return_minus_one_before_any_hip_call():
    """No GPU here: a call that got as far as a launch would return a positive hipError_t (or crash)."""
    lib = _lib.lib()
    buf = np.zeros(64, dtype=np.float64)                  # any non-null, 16-byte aligned host address: never dereferenced
    p = buf.ctypes.data
    assert p % 16 == 0
    ok = [p, 1, 4, p, p, 1, p, p, p, None]
    for k, bad, msg in ((0, None, b"null pointer"), (3, None, b"null pointer"), (4, None, b"null pointer"),
                        (6, None, b"null pointer"), (7, None, b"null pointer"), (8, None, b"null pointer"),
                        (1, 0, b"bad counts"), (1, -3, b"bad counts"), (5, 0, b"bad counts"), (5, -1, b"bad counts"),
                        (2, 0, b"bad counts"), (3, p + 4, b"16-byte aligned")):
        args = list(ok)
        args[k] = bad
        assert lib.codlad_stereo_check(*args) == -1, (k, bad)
        err = lib.codlad_last_error()
        assert b"codlad_stereo_check" in err and msg in err, (k, err)


def test_python_wrapper_rejects_cpu_tensors():
    top = template_topology(["ALA", "GLY", "SER"])
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        metrics.stereo_check(torch.zeros(1, top.n_atoms, 3), top)


def test_stereo_tables_on_every_template_and_two_chains():
    seq = sr.RES22 + ["PRO", "THR", "GLY"]
    ids = [0] * 12 + [1] * 13                              # LYS ends chain 0, MET starts chain 1
    top = template_topology(seq, chain_ids=ids)
    sites, kind = metrics.stereo_tables(top)
    assert sites.dtype == torch.int32 and tuple(sites.shape) == (25, 9, 4) and kind.dtype == torch.uint8 and tuple(kind.shape) == (25,)
    assert metrics.stereo_tables(top)[0] is sites          # built once, kept on the topology
    s = sites.numpy()
    exists = (s >= 0).all(-1)
    assert ((s >= 0).all(-1) | (s == -1).all(-1)).all() and s.max() < top.n_atoms
    n_chi = dict(ALA=0, GLY=0, SER=1, SEP=1, THR=1, TPO=1, CYS=1, VAL=1, ASN=2, ASP=2, HIS=2, ILE=2, LEU=2, PHE=2, PRO=2, TRP=2,
                 TYR=2, MET=3, GLN=3, GLU=3, ARG=4, LYS=4)
    assert set(n_chi) == set(sr.RES22)
    for r, nm in enumerate(seq):
        assert exists[r, 3:7].tolist() == [k < n_chi[nm] for k in range(4)], nm
        assert exists[r, 7] == (nm != "GLY"), nm
        assert exists[r, 8] == (nm in ("THR", "TPO", "ILE")), nm
        assert int(kind[r]) == (1 if nm == "PRO" else 0), nm
        first, last = r in (0, 12), r in (11, 24)
        assert exists[r, 0] == (not first) and exists[r, 2] == (not first) and exists[r, 1] == (not last), (r, nm)
    # the atoms, by name, against the reference's own table (written independently, tests/stereo_ref.py)
    assert np.array_equal(s, sr.site_index(top))
    name = lambda a: (int(top.residue_of_atom[a]), str(top.name[a]))                                        # noqa: E731
    r = seq.index("ILE")
    assert [name(a) for a in s[r, 4]] == [(r, "CA"), (r, "CB"), (r, "CG1"), (r, "CD1")]
    assert [name(a) for a in s[r, 8]] == [(r, "CB"), (r, "CA"), (r, "CG1"), (r, "CG2")]
    assert [name(a) for a in s[r, 2]] == [(r - 1, "CA"), (r - 1, "C"), (r, "N"), (r, "CA")]
    r = seq.index("MET")
    assert [name(a) for a in s[r, 5]] == [(r, "CB"), (r, "CG"), (r, "SD"), (r, "CE")]
    r = seq.index("THR")
    assert [name(a) for a in s[r, 8]] == [(r, "CB"), (r, "CA"), (r, "OG1"), (r, "CG2")]
    assert [name(a) for a in s[r, 7]] == [(r, "CA"), (r, "N"), (r, "C"), (r, "CB")]
    assert [name(a) for a in s[r, 1]] == [(r, "N"), (r, "CA"), (r, "C"), (r + 1, "N")]


def _args(**kw):
    base = dict(experiment="latent", model="diffusion", vae_type="N6", synthetic=False, pdb_files=None, data_process=False,
                fix_residues=None, superpose="none", cg_pdb=None, cg_xtc=None, geometry_check=False, stereo_check=True)
    return types.SimpleNamespace(**dict(base, **kw))


def test_cli_refuses_stereo_check_where_it_refuses_geometry_check():
    cli = cli_module()
    for ok in (_args(pdb_files=["a.pdb"]), _args(synthetic=True), _args(cg_pdb=["ca.pdb"]), _args(synthetic=True, experiment="recon"),
               _args(synthetic=True, data_process=True)):
        geo = types.SimpleNamespace(**dict(vars(ok), geometry_check=True))
        assert cli.check_cg_input(geo) is True and cli.check_stereo(ok) is True and ok.stereo_check is True
    off = _args(pdb_files=["a.pdb"], stereo_check=False)
    assert cli.check_stereo(off) is False and off.stereo_check is False
    assert cli.check_cg_input(_args(pdb_files=["a.pdb"])) is False               # it does not turn the geometry check on
    for change, reason in ((dict(data_process=True), "pickles carry none"), (dict(synthetic=True, experiment="bpd"), "generates none"),
                           (dict(synthetic=True, experiment="fmloss"), "generates none")):
        for check, flag in ((cli.check_stereo, "--stereo_check"), (cli.check_cg_input, "--geometry_check")):
            with pytest.raises(SystemExit) as e:
                check(_args(geometry_check=True, **change))
            assert reason in str(e.value) and flag in str(e.value), (change, str(e.value))
    with pytest.raises(SystemExit) as e:                     # with --cg_pdb the input route's own refusals come first
        cli.check_cg_input(_args(cg_pdb=["ca.pdb"], experiment="bpd"))
    assert "CA-only input has none" in str(e.value)


def test_pinned_torsion_ideal_volume_and_side_chain_sign():
    p = [np.array(v, dtype=np.float64) for v in ((1, 0, 0), (0, 0, 0), (0, 0, 1), (0, 1, 1))]
    assert sr.torsion(*p) == 90.0 and sr.torsion(*[q.astype(np.float32) for q in p]) == np.float32(90.0)
    assert sr.torsion(p[0], p[1], p[2], np.array([-1.0, 0, 1])) == 180.0                   # trans is +180, never -180
    assert np.isnan(sr.torsion(p[0], p[0], p[2], p[3])) and np.isnan(sr.torsion(p[0], p[1], p[1], p[3]))
    n = 6
    z = np.zeros(n)
    for d_ca, d_side in ((False, False), (True, False), (False, True)):
        top, xyz = sr.build_chain(["ALA", "THR", "ILE", "TPO", "GLY", "VAL"], z - 60, z - 45, z + 180, np.full((n, 4), -65.0),
                                  d_ca=[d_ca] * n, d_side=[d_side] * n)
        values, flags, counts = sr.reference(xyz, top)
        v_ca, v_side = values[0, :, 7], values[0, :, 8]
        sign = -1.0 if d_ca else 1.0
        assert np.isnan(v_ca[4]) and np.abs(np.delete(v_ca, 4) - sign * 2.509).max() < 1e-3, v_ca     # ideal L: +2.509 A^3
        assert np.isnan(v_side[[0, 4, 5]]).all()
        assert ((v_side[[1, 2, 3]] < -0.1) if d_side else (v_side[[1, 2, 3]] > 0.1)).all(), v_side     # natural THR / ILE: > 0
        assert counts[0].tolist() == [5 * d_ca, 3 * d_side, 0, 0, 0, 0]
        assert flags[0].tolist() == [sr.INVERTED_CA * (d_ca and i != 4) + sr.INVERTED_SIDE * (d_side and i in (1, 2, 3))
                                     for i in range(n)]


@pytest.mark.parametrize("n, breaks", [(3, ()), (65, ()), (257, ()), (90, (41,))])
def test_reference_returns_what_the_builder_planted(n, breaks):
    pl = sr.planted(n, 100 + n, breaks)
    top, xyz = sr.build_chain(**pl)
    values, flags, counts = sr.reference(xyz, top)
    tors, want_flags = sr.planted_truth(top, pl)
    assert np.array_equal(np.isnan(values[0, :, :7]), np.isnan(tors))
    assert np.nanmax(sr.angle_diff(values[0, :, :7], tors), initial=0.0) < 1e-9                     # NeRF round trip
    assert flags[0].tolist() == want_flags.tolist()
    assert counts[0, 5] == 0 and counts[0, 0] == int(((want_flags & sr.INVERTED_CA) > 0).sum())
    if breaks:
        b = breaks[0]
        assert np.isnan(values[0, b, [0, 2]]).all() and np.isnan(values[0, b - 1, 1]) and not np.isnan(values[0, b, 1])
