"""test.py with --relax and every analysis of its table on together, end to end on the device: the files each protein gets
are exactly those the table declares, the reports come in table order after the relax line, and the rows read the relaxed
coordinates.  The shapes are the four PED-length synthetic proteins, two frames, two members."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from codlad_amd import metrics, synth
from codlad_amd.utils.cg_input import template_topology
from tests.cli_script import ROOT, load_cli

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LENGTHS = (46, 87, 92, 129)
FLAGS = ("--relax 20 --geometry_check --stereo_check --observables 96 --saxs 16 --pr --cluster 1.0 --pca 3 --compare 20 --lddt "
         "--dssp").split()
# what the table declares but a dependent flag, absent here, writes
NOT_GIVEN = {"saxs_partials": "--saxs_hydration", "saxs_weights": "--saxs_reweight", "saxs_reweighted": "--saxs_reweight"}
# the opening titles of the reports, in table order
TITLES = ("geometry check (template topology, no true structure):",
          "stereo check (chirality, peptide bonds; geometry, not accuracy):",
          "ensemble observables (SASA in A^2, Rg in A, CA contacts at 8 A):",
          "SAXS profile (Debye sum, ensemble mean; q in 1/A):",
          "pair distribution P(r) (typed pair-distance histogram; A):",
          "clustering (Daura / GROMOS; RMSD in A):",
          "essential dynamics (mean structure, RMSF, PCA; A and A^2):",
          "generated against true ensemble (Jensen-Shannon divergences in bits, 0 = same distribution):",
          "lDDT of the generated structures against their true frames (1 = every local distance kept):",
          "secondary structure (DSSP, mean share of residues):")


def test_every_analysis_on_together(tmp_path):
    cli = load_cli("codlad_cli_all")
    cmd = [sys.executable, os.path.join(ROOT, "test.py"), "--synthetic", "--synthetic_weights", "--synthetic_frames", "2",
           "--num_ensemble", "2", "--num_sampling_steps", "4"] + FLAGS
    res = subprocess.run(cmd, env=dict(os.environ, PYTHONPATH=ROOT), cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-1500:] + res.stderr[-3000:]
    files = {f: os.path.join(dp, f) for dp, _d, fs in os.walk(os.path.join(str(tmp_path), "logs")) for f in fs}
    declared = [suffix for row in cli.ANALYSES for suffix, _get in row.writes]
    assert len(declared) == len(set(declared)) and set(NOT_GIVEN) < set(declared)
    want = (set(declared) - set(NOT_GIVEN)) | {"xyz_recon", "xyz_unrelaxed", "relax"}
    assert set(files) == {f"synthetic_L{L}_{suffix}.npy" for L in LENGTHS for suffix in want}
    lines = res.stdout.splitlines()
    for i, L in enumerate(LENGTHS):
        name = f"synthetic_L{L}"
        # the reports of this protein: from its relax line to its closing line, every opening title once and in table order
        first = next(k for k, line in enumerate(lines) if line.startswith(f"relax {name}: 20 iterations"))
        last = next(k for k, line in enumerate(lines) if line.startswith(f"{name}: 2 frames x 2 members"))
        opened = [line[len("############## vvvvvvvvv "):] for line in lines[first:last] if line.startswith("############## vvvvvvvvv ")]
        assert opened == list(TITLES), (name, opened)
        # every row saw the relaxed coordinates: what is written beside them follows from them, to the bit
        xyz = np.load(files[f"{name}_xyz_recon.npy"])
        assert xyz.shape[:2] == (2, 2)
        prot = synth.make_protein(L, 1000 + i, n_frames=2, phospho=False)
        top = template_topology([synth.IDX2THR[int(z)] for z in prot["z_full"]][1:-1])
        pool = torch.from_numpy(xyz).to(DEV).reshape(-1, xyz.shape[2], 3)
        geo = metrics.geometry_check(pool, top, order=2, near_dist=9.0)
        assert np.array_equal(geo["counts"].cpu().numpy(), np.load(files[f"{name}_geometry.npy"]))
        assert np.array_equal(geo["min_dist"].cpu().numpy(), np.load(files[f"{name}_geometry_min.npy"]))
        assert np.array_equal(metrics.dssp(pool, top)["ss"].cpu().numpy(), np.load(files[f"{name}_dssp.npy"]))
