"""CA-only input (codlad_amd/utils/cg_input.py, test.py --cg_pdb / --cg_xtc): a coarse-grained trajectory must give the
sampling path exactly what the all-atom route gives it - the same batch tensors, the same info tables and, through the CLI,
bit-identical generated coordinates - without ever holding an atom besides the CAs.

The CPU tests hold the reader, the template topology and the flag checks; the GPU tests build both routes from one golden
(N6_L46_B3: 46 residues, 3 frames) and run the CLI once per route (a module fixture shared by the tests that read its
output, the geometry files among them)."""
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

from tests import cases
from tests.test_dataset_builder import golden_frames, write_full_pdb
from codlad_amd import synth
from codlad_amd.utils import cg_input
from codlad_amd.utils import dataset_builder as db
from codlad_amd.utils.ic_tables import PDB_ATOM_ORDER
from codlad_amd.utils.protein_module import info_from_residues
from codlad_amd.utils.xtc import read_xtc, write_xtc
from tests.cli_script import load_cli

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAMS = {"atom_cutoff": 9.0, "cg_cutoff": 21.0, "edgeorder": 2}


def cli_module():
    return load_cli("codlad_cli_cg")


def strip_to_ca(src, dst, keep=lambda line: True):
    with open(src) as f, open(dst, "w") as g:
        for line in f:
            if line[:6] in ("ATOM  ", "HETATM") and (line[12:16].strip() != "CA" or not keep(line)):
                continue
            g.write(line)


def snapped_frames(top, full, tmp):
    """The golden's frames with every CA moved (by < 0.05 A) onto a coordinate that a %8.3f PDB field and the .xtc's 1e-3 nm
    grid decode to the SAME float32, so that the PDB and the xtc route can be compared bit for bit; all other atoms on the
    PDB's 1e-3 A grid.  Found by writing and re-reading an .xtc, never by running the code under test."""
    ca = top.select("CA")
    k = np.round(full[:, ca].astype(np.float64) * 100).astype(np.int64)              # CA coordinates in 0.01 A = 1e-3 nm
    path = os.path.join(tmp, "snap.xtc")
    for _ in range(8):
        write_xtc(path, k / 100.0)
        from_xtc = read_xtc(path)[0]
        from_pdb = np.array([[[float(f"{v / 100.0:8.3f}") for v in atom] for atom in fr] for fr in k], dtype=np.float32)
        differ = from_xtc != from_pdb
        if not differ.any():
            break
        k[differ] += 1
    assert not differ.any(), "no common grid found"
    out = np.round(full.astype(np.float64), 3)
    out[:, ca] = k / 100.0
    return out, from_pdb


# ---------------------------------------------------------------------------------------------------------- CPU: reader
def test_all_atom_file_and_its_ca_strip_read_the_same(tmp_path):
    top, full, _og, _info, _g5 = golden_frames("N6_L46_B3")
    write_full_pdb(str(tmp_path / "full.pdb"), top, full, chain_breaks=(20,))
    strip_to_ca(str(tmp_path / "full.pdb"), str(tmp_path / "ca.pdb"))
    seq_a, xyz_a = cg_input.read_cg_pdb(str(tmp_path / "full.pdb"))
    seq_b, xyz_b = cg_input.read_cg_pdb(str(tmp_path / "ca.pdb"))
    assert seq_a == seq_b and xyz_a.dtype == np.float32 and np.array_equal(xyz_a, xyz_b)
    assert xyz_a.shape == (3, 48, 3)
    assert list(seq_a.res_names) == top.res_names and list(seq_a.res_seqs) == list(range(1, 49))
    assert list(seq_a.chain_ids) == [0] * 20 + [1] * 28                         # numbered in order of appearance
    _top2, frames = db.read_pdb(str(tmp_path / "full.pdb"))                     # the same floats read_pdb takes from the file
    assert np.array_equal(xyz_a, frames[:, top.select("CA")])
    with open(str(tmp_path / "ca.pdb")) as f:
        assert sum(line.startswith("ATOM") for line in f) == 3 * 48


def test_reader_names_the_offending_residue(tmp_path):
    top, full, _og, _info, _g5 = golden_frames("N6_L46_B3")
    src = str(tmp_path / "full.pdb")
    write_full_pdb(src, top, full[:2])
    lines = open(src).read().splitlines(True)

    def variant(name, edit):
        path = str(tmp_path / name)
        with open(path, "w") as g:
            g.writelines(edit(list(lines)))
        return path

    nm5 = top.res_names[4]
    is_res5 = lambda l: l.startswith("ATOM") and int(l[22:26]) == 5                                  # noqa: E731
    first_model_end = next(i for i, l in enumerate(lines) if l.startswith("ENDMDL"))
    unknown = variant("unknown.pdb", lambda ls: [l[:17] + "XYZ" + l[20:] if is_res5(l) else l for l in ls])
    with pytest.raises(ValueError, match=r"XYZ 5 .*no template"):
        cg_input.read_cg_pdb(unknown)
    no_ca = variant("no_ca.pdb", lambda ls: [l for l in ls if not (is_res5(l) and l[12:16].strip() == "CA")])
    with pytest.raises(ValueError, match=rf"{nm5} 5 .*has 0 CA"):
        cg_input.read_cg_pdb(no_ca)
    two_ca = variant("two_ca.pdb", lambda ls: [x for l in ls for x in ([l, l] if is_res5(l) and l[12:16].strip() == "CA" else [l])])
    with pytest.raises(ValueError, match=rf"{nm5} 5 .*has 2 CA"):
        cg_input.read_cg_pdb(two_ca)
    short = variant("short.pdb", lambda ls: [l for i, l in enumerate(ls) if not (i > first_model_end and is_res5(l))])
    with pytest.raises(ValueError, match=r"model 2 has 47 CA atoms, the first has 48"):
        cg_input.read_cg_pdb(short)
    # an alternate location B is ignored, A is read: no doubled CA
    alt = variant("alt.pdb", lambda ls: [x for l in ls for x in ([l[:16] + "A" + l[17:], l[:16] + "B" + l[17:]]
                                                                  if is_res5(l) and l[12:16].strip() == "CA" else [l])])
    assert np.array_equal(cg_input.read_cg_pdb(alt)[1], cg_input.read_cg_pdb(src)[1])


def test_xtc_frames_need_one_atom_per_ca(tmp_path):
    top, full, _og, _info, _g5 = golden_frames("N6_L46_B3")
    write_full_pdb(str(tmp_path / "full.pdb"), top, full)
    ca = full[:, top.select("CA")]
    write_xtc(str(tmp_path / "ok.xtc"), ca)
    write_xtc(str(tmp_path / "bad.xtc"), ca[:, :-1])
    seq, xyz = cg_input.load_cg_frames(str(tmp_path / "full.pdb"), str(tmp_path / "ok.xtc"))
    assert xyz.shape == (3, 48, 3) and np.abs(xyz - ca).max() < 6e-3 and list(seq.res_names) == top.res_names
    with pytest.raises(ValueError, match="47 atoms.*48 CA"):
        cg_input.load_cg_frames(str(tmp_path / "full.pdb"), str(tmp_path / "bad.xtc"))


# ------------------------------------------------------------------------------------------- CPU: template topology
def test_pdb_atom_order_is_product_code_and_still_importable_from_synth():
    assert synth.PDB_ATOM_ORDER is PDB_ATOM_ORDER
    import inspect
    assert "synth" not in inspect.getsource(cg_input)


@pytest.mark.parametrize("name", list(cases.INFO_CASES))
def test_template_topology_gives_the_reference_info_tables(name):
    n_cg, seed, phospho = cases.INFO_CASES[name]
    gold = np.load(cases.npz_path(f"g13_info_{name}"))
    names = [synth.IDX2THR[int(z)] for z in synth.sequence(n_cg + 2, 2000 + seed, phospho=phospho)]
    top = cg_input.template_topology(names)
    assert top.res_names == names and top.n_residues == n_cg + 2
    (permute, atom_idx, orders), n = info_from_residues(top.res_names, top.atom_names)
    # the goldens' file order is the template order: the tables are equal as they stand (no permutation to undo)
    assert n == int(gold["n_cg"])
    assert np.array_equal(permute.numpy(), gold["permute"]) and np.array_equal(atom_idx.numpy(), gold["atom_idx"])
    assert np.array_equal(orders.numpy(), gold["atom_orders"])
    with pytest.raises(ValueError, match="HOH has no template"):
        cg_input.template_topology(names[:3] + ["HOH"])


def test_template_topology_bond_counts():
    top, _full, _og, _info, _g5 = golden_frames("N6_L46_B3")
    tt = cg_input.template_topology(top.res_names, top.res_seqs, top.chain_ids)
    inner = tt.subset_residues(1, tt.n_residues - 1)
    assert inner.atom_names == top.atom_names[1:-1]
    bonds = db.standard_bonds(inner)
    # a chain is a tree plus one extra bond per ring (PRO, PHE, TYR, HIS: 1; TRP: 2)
    rings = sum({"PRO": 1, "PHE": 1, "TYR": 1, "HIS": 1, "TRP": 2}.get(nm, 0) for nm in inner.res_names)
    assert bonds.shape[0] == inner.n_atoms - 1 + rings and bonds.shape[0] > 300
    assert (bonds[:, 0] < bonds[:, 1]).all()
    assert list(inner.element) == [a[0] for a in inner.name] and set(inner.atomic_nums()) <= {6, 7, 8, 16, 15}
    two = cg_input.template_topology(top.res_names, chain_ids=[0] * 20 + [1] * 28).subset_residues(1, 47)
    assert db.standard_bonds(two).shape[0] == bonds.shape[0] - 1                 # no peptide bond across the chain break


# ------------------------------------------------------------------------------------------------- CPU: flag conflicts
def _args(**kw):
    base = dict(experiment="latent", model="diffusion", vae_type="N6", synthetic=False, pdb_files=None, data_process=False,
                fix_residues=None, superpose="none", cg_pdb=["ca.pdb"], cg_xtc=None, geometry_check=False)
    return types.SimpleNamespace(**dict(base, **kw))


def test_flag_conflicts_exit_with_their_reason():
    cli = cli_module()
    ok = _args()
    assert cli.check_cg_input(ok) is True and ok.geometry_check is True          # implied by --cg_pdb
    for model in ("fm", "icfm"):
        assert cli.check_cg_input(_args(model=model)) is True
    off = _args(cg_pdb=None, pdb_files=["a.pdb"])
    assert cli.check_cg_input(off) is False and off.geometry_check is False      # today's runs stay as they are
    assert cli.check_cg_input(_args(cg_pdb=None, pdb_files=["a.pdb"], geometry_check=True)) is True
    assert cli.check_cg_input(_args(cg_xtc="t.xtc")) is True
    for change, reason in ((dict(experiment="recon"), "encodes the input's atoms"),
                           (dict(experiment="genzprot"), "--experiment latent"),
                           (dict(experiment="bpd"), "CA-only input has none"),
                           (dict(experiment="fmloss"), "CA-only input has none"),
                           (dict(fix_residues="3-5"), "--fix_residues"),
                           (dict(superpose="ref"), "--superpose ref"),
                           (dict(cg_xtc="t.xtc", cg_pdb=["a.pdb", "b.pdb"]), "single --cg_pdb"),
                           (dict(cg_xtc="t.xtc", cg_pdb=None), "--cg_xtc needs --cg_pdb"),
                           (dict(pdb_files=["a.pdb"]), "input route of its own"),
                           (dict(synthetic=True), "input route of its own"),
                           (dict(cg_pdb=None, data_process=True, geometry_check=True), "pickles carry none"),
                           (dict(cg_pdb=None, synthetic=True, experiment="bpd", geometry_check=True), "generates none")):
        with pytest.raises(SystemExit) as e:
            cli.check_cg_input(_args(**change))
        assert reason in str(e.value), (change, str(e.value))


def test_cli_documents_the_lost_termini():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "test.py"), "--help"], capture_output=True, text=True,
                         env=dict(os.environ, PYTHONPATH=ROOT), timeout=300)
    text = " ".join(out.stdout.split())
    assert out.returncode == 0 and "--cg_pdb" in text and "--cg_xtc" in text and "--geometry_check" in text
    assert "loses its first and last residue" in text


# ------------------------------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def routes(tmp_path_factory):
    """full.pdb (all atoms, template order), ca.pdb (its CA lines), ca.xtc (the same CAs), on a grid all three agree on;
    then the CLI once per route.  -> dict: directory, topology, frames and the three runs' (files, stdout)."""
    tmp = str(tmp_path_factory.mktemp("cg_routes"))
    top, full, _og, info, _g5 = golden_frames("N6_L46_B3")
    frames, ca = snapped_frames(top, full, tmp)
    write_full_pdb(os.path.join(tmp, "full.pdb"), top, frames)
    strip_to_ca(os.path.join(tmp, "full.pdb"), os.path.join(tmp, "ca.pdb"))
    write_xtc(os.path.join(tmp, "ca.xtc"), ca)
    runs = {}
    common = ["--synthetic_weights", "--num_sampling_steps", "5", "--num_ensemble", "2", "--seed", "7"]
    for key, extra in (("pdb", ["--pdb_files", "full.pdb"]), ("cg", ["--cg_pdb", "ca.pdb"]),
                       ("xtc", ["--cg_pdb", "ca.pdb", "--cg_xtc", "ca.xtc", "--save_pdb", "--superpose", "first", "--save_codes"])):
        cwd = os.path.join(tmp, key)
        os.makedirs(cwd)
        out = subprocess.run([sys.executable, os.path.join(ROOT, "test.py")] + common +
                             [os.path.join("..", a) if a.endswith((".pdb", ".xtc")) else a for a in extra],
                             cwd=cwd, env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
        files = {f: os.path.join(dp, f) for dp, _d, fs in os.walk(os.path.join(cwd, "logs")) for f in fs}
        runs[key] = (files, out.stdout)
    return dict(tmp=tmp, top=top, info=info, ca=ca, runs=runs)


@pytest.mark.gpu
def test_both_routes_build_the_same_batches(routes):
    from codlad_amd.utils.dataset_module import load_dataset
    tmp = routes["tmp"]
    loader, info_dict, _n_atoms, n_cgs, _z, inner = load_dataset(os.path.join(tmp, "full"), PARAMS, device="cuda")
    want = list(loader)
    seq, ca_xyz = cg_input.read_cg_pdb(os.path.join(tmp, "ca.pdb"))
    assert np.array_equal(ca_xyz, routes["ca"])
    top = cg_input.template_topology(*seq)
    got = list(cg_input.cg_batches(top, ca_xyz, PARAMS, device="cuda"))
    assert len(got) == len(want) == 1 and n_cgs == 48
    batch, info = got[0]
    assert set(batch) == {"CG_nxyz", "OG_CG_nxyz", "num_CGs", "CG_nbr_list", "prot_idx"}
    cli = cli_module()
    assert not set(batch) & set(cli.EVAL_KEYS)
    for k in batch:
        assert batch[k].dtype == want[0][k].dtype and torch.equal(batch[k], want[0][k]), k
    assert batch["CG_nbr_list"].shape[0] > 100
    for a, b, c in zip(info, info_dict[0], routes["info"]):
        assert torch.equal(a, b) and torch.equal(a, c)
    assert top.subset_residues(1, 47).atom_names == inner.atom_names
    seq_x, ca_x = cg_input.load_cg_frames(os.path.join(tmp, "ca.pdb"), os.path.join(tmp, "ca.xtc"))
    assert seq_x == seq and np.array_equal(ca_x, ca_xyz)                          # the common grid of the fixture


@pytest.mark.gpu
def test_cli_routes_generate_bit_identical_structures(routes):
    runs = routes["runs"]
    a = np.load(runs["pdb"][0]["full_xyz_recon.npy"])
    b = np.load(runs["cg"][0]["ca_xyz_recon.npy"])
    c = np.load(runs["xtc"][0]["ca_xyz_recon.npy"])
    n_atoms = routes["top"].n_atoms - 2
    assert a.shape == (2, 3, n_atoms, 3) and np.isfinite(a).all()
    assert a.tobytes() == b.tobytes()
    assert a.tobytes() == c.tobytes()
    assert not np.array_equal(a[0], a[1])                                          # two members, two samples


@pytest.mark.gpu
def test_cli_output_files(routes):
    from codlad_amd import metrics
    runs = routes["runs"]
    # without --geometry_check the --pdb_files route writes what it wrote before, and prints its Evaluation block
    assert set(runs["pdb"][0]) == {"full_xyz_recon.npy"}
    assert "test_all_valid_ratio" in runs["pdb"][1] and "geometry" not in runs["pdb"][1]
    files, stdout = runs["cg"]
    assert set(files) == {"ca_xyz_recon.npy", "ca_geometry.npy", "ca_geometry_min.npy"}
    assert "test_all_valid_ratio" not in stdout and "result test_stats" not in stdout      # nothing to compare with
    for word in ("geometry_valid_ratio", "geometry_broken_bonds", "geometry_spurious_bonds", "geometry_clashes",
                 "geometry_clash_over_near", "geometry_min_dist"):
        assert word in stdout, word
    geo, gmin = np.load(files["ca_geometry.npy"]), np.load(files["ca_geometry_min.npy"])
    xyz = np.load(files["ca_xyz_recon.npy"])
    assert geo.dtype == np.int32 and geo.shape == (2 * 3, 5) and gmin.shape == (6,) and gmin.dtype == np.float32
    top = cg_input.template_topology(routes["top"].res_names).subset_residues(1, 47)
    by_hand = metrics.geometry_check(torch.from_numpy(xyz).cuda().reshape(6, -1, 3), top)
    assert np.array_equal(geo[:, 2], by_hand["bonded"].cpu().numpy())
    assert np.array_equal(geo, by_hand["counts"].cpu().numpy()) and np.array_equal(gmin, by_hand["min_dist"].cpu().numpy())
    n_bonds = db.standard_bonds(top).shape[0]
    assert np.array_equal(geo[:, 2], n_bonds - geo[:, 0] + geo[:, 1])
    # --save_pdb / .xtc / --superpose first / --save_codes go through the template atom names
    files = runs["xtc"][0]
    assert {"generated_traj_ca.pdb", "generated_traj_ca.xtc", "ca_codes.npy", "ca_geometry.npy"} <= set(files)
    top2, written = db.read_pdb(files["generated_traj_ca.pdb"])
    assert top2.atom_names == top.atom_names and top2.res_names == top.res_names and written.shape == (6, top.n_atoms, 3)
    assert np.abs(written[:3] - xyz[0]).max() < 6e-4                              # member 0 is what the others are moved onto
    assert np.load(files["ca_codes.npy"]).shape == (6, 46)


@pytest.mark.gpu
def test_clash_ratio_equals_the_pinned_clash_metric(routes):
    """clash / near of the geometry check = metrics.clash_result (the reference's first clash term) fed the structure's own
    neighbour list, the order-2 edge list of the template topology and no backbone N..O list."""
    from codlad_amd import metrics
    xyz = torch.from_numpy(np.load(routes["runs"]["cg"][0]["ca_xyz_recon.npy"])).cuda().reshape(6, -1, 3)
    top = cg_input.template_topology(routes["top"].res_names).subset_residues(1, 47)
    edges = db.high_order_edges(db.standard_bonds(top), 2, top.n_atoms).cuda()
    geo = metrics.geometry_check(xyz, top, order=2, near_dist=9.0)
    empty = torch.zeros(0, 2, dtype=torch.int64, device="cuda")
    for s in range(6):
        nbr = db.neighbor_list(xyz[s], 9.0)
        want = float(metrics.clash_result(edges, nbr, xyz[s], empty))
        got = float(geo["clash"][s].to(torch.float32) / geo["near"][s].to(torch.float32))
        print(f"structure {s}: clash {int(geo['clash'][s])} near {int(geo['near'][s])} ratio {got:.9g} clash_result {want:.9g}")
        assert abs(got - want) <= 1e-6 * abs(want), (s, got, want)
