"""Which refusal a command line gets: build_parser().parse_args(argv) followed by check_args(args) either returns (None
below) or raises SystemExit with exactly the recorded text.  The texts were recorded from the script as it stood before the
analyses became rows of one table, by running it as a subprocess on a machine without a GPU: a refusal exits before the GPU
is asked for, an accepted line ends in "needs an MI355X: there is no CPU path".  Nothing here starts the script: on a GPU
machine an accepted line would go on to run.

For every analysis flag, --relax and the dependent flags: the flag alone on the synthetic route, with --experiment bpd,
with --experiment fmloss, on the pickle route, on the CA-only route; one value on each side of every bound a check states;
each dependent flag without its parent; and lines with two faults, which pin the order of the checks."""
import pytest

from tests.cli_script import load_cli

CLI = load_cli("codlad_cli_refusals")

CASES = (
    ('--geometry_check --synthetic', None),
    ('--geometry_check --synthetic --experiment bpd', '--geometry_check judges generated structures: --experiment bpd generates none'),
    ('--geometry_check --synthetic --experiment fmloss', '--geometry_check judges generated structures: --experiment fmloss generates none'),
    ('--geometry_check --data_process', '--geometry_check needs the topology of the structures: --data_process pickles carry none (use --pdb_files, --cg_pdb or --synthetic)'),
    ('--geometry_check --cg_pdb x.pdb', None),
    ('--stereo_check --synthetic', None),
    ('--stereo_check --synthetic --experiment bpd', '--stereo_check judges generated structures: --experiment bpd generates none'),
    ('--stereo_check --synthetic --experiment fmloss', '--stereo_check judges generated structures: --experiment fmloss generates none'),
    ('--stereo_check --data_process', '--stereo_check needs the topology of the structures: --data_process pickles carry none (use --pdb_files, --cg_pdb or --synthetic)'),
    ('--stereo_check --cg_pdb x.pdb', None),
    ('--relax --synthetic', None),
    ('--relax --synthetic --experiment bpd', '--relax relaxes generated structures: --experiment bpd generates none'),
    ('--relax --synthetic --experiment fmloss', '--relax relaxes generated structures: --experiment fmloss generates none'),
    ('--relax --data_process', '--relax needs the topology of the structures: --data_process pickles carry none (use --pdb_files, --cg_pdb or --synthetic)'),
    ('--relax --cg_pdb x.pdb', None),
    ('--relax 20 --synthetic', None),
    ('--relax 20 --synthetic --experiment bpd', '--relax relaxes generated structures: --experiment bpd generates none'),
    ('--relax 20 --synthetic --experiment fmloss', '--relax relaxes generated structures: --experiment fmloss generates none'),
    ('--relax 20 --data_process', '--relax needs the topology of the structures: --data_process pickles carry none (use --pdb_files, --cg_pdb or --synthetic)'),
    ('--relax 20 --cg_pdb x.pdb', None),
    ('--observables --synthetic', None),
    ('--observables --synthetic --experiment bpd', '--observables describes generated structures: --experiment bpd generates none'),
    ('--observables --synthetic --experiment fmloss', '--observables describes generated structures: --experiment fmloss generates none'),
    ('--observables --data_process', '--observables needs the topology of the structures: --data_process pickles carry none (use --pdb_files, --cg_pdb or --synthetic)'),
    ('--observables --cg_pdb x.pdb', None),
    ('--saxs --synthetic', None),
    ('--saxs --synthetic --experiment bpd', '--saxs describes generated structures: --experiment bpd generates none'),
    ('--saxs --synthetic --experiment fmloss', '--saxs describes generated structures: --experiment fmloss generates none'),
    ('--saxs --data_process', '--saxs needs the topology of the structures: --data_process pickles carry none (use --pdb_files, --cg_pdb or --synthetic)'),
    ('--saxs --cg_pdb x.pdb', None),
    ('--pr --synthetic', None),
    ('--pr --synthetic --experiment bpd', '--pr describes generated structures: --experiment bpd generates none'),
    ('--pr --synthetic --experiment fmloss', '--pr describes generated structures: --experiment fmloss generates none'),
    ('--pr --data_process', '--pr needs the topology of the structures: --data_process pickles carry none (use --pdb_files, --cg_pdb or --synthetic)'),
    ('--pr --cg_pdb x.pdb', None),
    ('--cluster 1.0 --synthetic', None),
    ('--cluster 1.0 --synthetic --experiment bpd', '--cluster describes generated structures: --experiment bpd generates none'),
    ('--cluster 1.0 --synthetic --experiment fmloss', '--cluster describes generated structures: --experiment fmloss generates none'),
    ('--cluster 1.0 --data_process', None),
    ('--cluster 1.0 --cg_pdb x.pdb', None),
    ('--pca --synthetic', None),
    ('--pca --synthetic --experiment bpd', '--pca describes generated structures: --experiment bpd generates none'),
    ('--pca --synthetic --experiment fmloss', '--pca describes generated structures: --experiment fmloss generates none'),
    ('--pca --data_process', None),
    ('--pca --cg_pdb x.pdb', None),
    ('--compare --synthetic', None),
    ('--compare --synthetic --experiment bpd', '--compare compares generated structures with the true ones: --experiment bpd generates none'),
    ('--compare --synthetic --experiment fmloss', '--compare compares generated structures with the true ones: --experiment fmloss generates none'),
    ('--compare --data_process', None),
    ('--compare --cg_pdb x.pdb', None),
    ('--lddt --synthetic', None),
    ('--lddt --synthetic --experiment bpd', '--lddt scores generated structures against the true ones: --experiment bpd generates none'),
    ('--lddt --synthetic --experiment fmloss', '--lddt scores generated structures against the true ones: --experiment fmloss generates none'),
    ('--lddt --data_process', None),
    ('--lddt --cg_pdb x.pdb', None),
    ('--dssp --synthetic', None),
    ('--dssp --synthetic --experiment bpd', '--dssp describes generated structures: --experiment bpd generates none'),
    ('--dssp --synthetic --experiment fmloss', '--dssp describes generated structures: --experiment fmloss generates none'),
    ('--dssp --data_process', '--dssp needs the topology of the structures: --data_process pickles carry none (use --pdb_files, --cg_pdb or --synthetic)'),
    ('--dssp --cg_pdb x.pdb', None),
    # the dependent flags with their parents, on the same five routes
    ('--saxs 16 --saxs_data curve.dat --synthetic', None),
    ('--saxs 16 --saxs_data curve.dat --synthetic --experiment bpd', '--saxs describes generated structures: --experiment bpd generates none'),
    ('--saxs 16 --saxs_data curve.dat --synthetic --experiment fmloss', '--saxs describes generated structures: --experiment fmloss generates none'),
    ('--saxs 16 --saxs_data curve.dat --data_process', '--saxs needs the topology of the structures: --data_process pickles carry none (use --pdb_files, --cg_pdb or --synthetic)'),
    ('--saxs 16 --saxs_data curve.dat --cg_pdb x.pdb', None),
    ('--saxs 16 --saxs_hydration 1.0 0.5 --synthetic', None),
    ('--saxs 16 --saxs_hydration 1.0 0.5 --synthetic --experiment bpd', '--saxs describes generated structures: --experiment bpd generates none'),
    ('--saxs 16 --saxs_hydration 1.0 0.5 --synthetic --experiment fmloss', '--saxs describes generated structures: --experiment fmloss generates none'),
    ('--saxs 16 --saxs_hydration 1.0 0.5 --data_process', '--saxs needs the topology of the structures: --data_process pickles carry none (use --pdb_files, --cg_pdb or --synthetic)'),
    ('--saxs 16 --saxs_hydration 1.0 0.5 --cg_pdb x.pdb', None),
    ('--saxs 16 --saxs_data curve.dat --saxs_hydration --synthetic', None),
    ('--saxs 16 --saxs_data curve.dat --saxs_hydration --synthetic --experiment bpd', '--saxs describes generated structures: --experiment bpd generates none'),
    ('--saxs 16 --saxs_data curve.dat --saxs_hydration --synthetic --experiment fmloss', '--saxs describes generated structures: --experiment fmloss generates none'),
    ('--saxs 16 --saxs_data curve.dat --saxs_hydration --data_process', '--saxs needs the topology of the structures: --data_process pickles carry none (use --pdb_files, --cg_pdb or --synthetic)'),
    ('--saxs 16 --saxs_data curve.dat --saxs_hydration --cg_pdb x.pdb', None),
    ('--saxs 16 --saxs_data curve.dat --saxs_reweight 10 1 --synthetic', None),
    ('--saxs 16 --saxs_data curve.dat --saxs_reweight 10 1 --synthetic --experiment bpd', '--saxs describes generated structures: --experiment bpd generates none'),
    ('--saxs 16 --saxs_data curve.dat --saxs_reweight 10 1 --synthetic --experiment fmloss', '--saxs describes generated structures: --experiment fmloss generates none'),
    ('--saxs 16 --saxs_data curve.dat --saxs_reweight 10 1 --data_process', '--saxs needs the topology of the structures: --data_process pickles carry none (use --pdb_files, --cg_pdb or --synthetic)'),
    ('--saxs 16 --saxs_data curve.dat --saxs_reweight 10 1 --cg_pdb x.pdb', None),
    ('--compare --compare_cluster 2.0 --synthetic', None),
    ('--compare --compare_cluster 2.0 --synthetic --experiment bpd', '--compare compares generated structures with the true ones: --experiment bpd generates none'),
    ('--compare --compare_cluster 2.0 --synthetic --experiment fmloss', '--compare compares generated structures with the true ones: --experiment fmloss generates none'),
    ('--compare --compare_cluster 2.0 --data_process', None),
    ('--compare --compare_cluster 2.0 --cg_pdb x.pdb', None),
    ('--pca --pca_atoms all --synthetic', None),
    ('--pca --pca_atoms all --synthetic --experiment bpd', '--pca describes generated structures: --experiment bpd generates none'),
    ('--pca --pca_atoms all --synthetic --experiment fmloss', '--pca describes generated structures: --experiment fmloss generates none'),
    ('--pca --pca_atoms all --data_process', None),
    ('--pca --pca_atoms all --cg_pdb x.pdb', None),
    ('--cluster 1.0 --cluster_atoms all --synthetic', None),
    ('--cluster 1.0 --cluster_atoms all --synthetic --experiment bpd', '--cluster describes generated structures: --experiment bpd generates none'),
    ('--cluster 1.0 --cluster_atoms all --synthetic --experiment fmloss', '--cluster describes generated structures: --experiment fmloss generates none'),
    ('--cluster 1.0 --cluster_atoms all --data_process', None),
    ('--cluster 1.0 --cluster_atoms all --cg_pdb x.pdb', None),
    # one value on each side of every bound
    ('--relax -1 --synthetic', '--relax takes a number of iterations >= 0, got -1'),
    ('--relax 0 --synthetic', None),
    ('--observables 0 --synthetic', '--observables takes a number of test points per atom in 1 .. 1024, got 0'),
    ('--observables 1 --synthetic', None),
    ('--observables 1024 --synthetic', None),
    ('--observables 1025 --synthetic', '--observables takes a number of test points per atom in 1 .. 1024, got 1025'),
    ('--saxs 0 --synthetic', '--saxs takes a number of q values in 1 .. 512, got 0'),
    ('--saxs 1 --synthetic', None),
    ('--saxs 512 --synthetic', None),
    ('--saxs 513 --synthetic', '--saxs takes a number of q values in 1 .. 512, got 513'),
    ('--pr 0 --synthetic', '--pr takes a bin width in A, a positive number, got 0.0'),
    ('--pr 0.001 --synthetic', None),
    ('--pr -1 --synthetic', '--pr takes a bin width in A, a positive number, got -1.0'),
    ('--pr nan --synthetic', '--pr takes a bin width in A, a positive number, got nan'),
    ('--pr inf --synthetic', '--pr takes a bin width in A, a positive number, got inf'),
    ('--cluster 0 --synthetic', '--cluster takes an RMSD cut-off in A, a positive number, got 0.0'),
    ('--cluster 0.001 --synthetic', None),
    ('--cluster -1 --synthetic', '--cluster takes an RMSD cut-off in A, a positive number, got -1.0'),
    ('--cluster nan --synthetic', '--cluster takes an RMSD cut-off in A, a positive number, got nan'),
    ('--cluster inf --synthetic', '--cluster takes an RMSD cut-off in A, a positive number, got inf'),
    ('--pca 0 --synthetic', '--pca takes the number of components, 1 .. 64, got 0'),
    ('--pca 1 --synthetic', None),
    ('--pca 64 --synthetic', None),
    ('--pca 65 --synthetic', '--pca takes the number of components, 1 .. 64, got 65'),
    ('--compare 0 --synthetic', '--compare takes the number of distance bins, 1 .. 256, got 0'),
    ('--compare 1 --synthetic', None),
    ('--compare 256 --synthetic', None),
    ('--compare 257 --synthetic', '--compare takes the number of distance bins, 1 .. 256, got 257'),
    ('--compare --compare_cluster 0 --synthetic', '--compare_cluster takes an RMSD cut-off in A, a positive number, got 0.0'),
    ('--compare --compare_cluster 0.001 --synthetic', None),
    ('--compare --compare_cluster nan --synthetic', '--compare_cluster takes an RMSD cut-off in A, a positive number, got nan'),
    ('--compare --compare_cluster inf --synthetic', '--compare_cluster takes an RMSD cut-off in A, a positive number, got inf'),
    ('--saxs 16 --saxs_hydration 1.0 --synthetic', '--saxs_hydration takes C1 and C2 or nothing (then both are fitted to --saxs_data), got 1 number(s)'),
    ('--saxs 16 --saxs_hydration 1 2 3 --synthetic', '--saxs_hydration takes C1 and C2 or nothing (then both are fitted to --saxs_data), got 3 number(s)'),
    ('--saxs 16 --saxs_hydration 0 0.5 --synthetic', '--saxs_hydration: C1 scales the excluded volume and must be positive, C2 a number, got 0.0 0.5'),
    ('--saxs 16 --saxs_hydration 0.001 0.5 --synthetic', None),
    ('--saxs 16 --saxs_hydration 1.0 nan --synthetic', '--saxs_hydration: C1 scales the excluded volume and must be positive, C2 a number, got 1.0 nan'),
    ('--saxs 16 --saxs_hydration --synthetic', '--saxs_hydration without C1 and C2 fits them: that needs the curve of --saxs_data'),
    ('--saxs 16 --saxs_data curve.dat --saxs_reweight --synthetic', '--saxs_reweight takes one THETA or more (the confidence in the prior; try 1000 100 10 1)'),
    ('--saxs 16 --saxs_data curve.dat --saxs_reweight 0 --synthetic', '--saxs_reweight: every THETA must be a positive finite number, got 0.0'),
    ('--saxs 16 --saxs_data curve.dat --saxs_reweight 0.001 --synthetic', None),
    ('--saxs 16 --saxs_data curve.dat --saxs_reweight 10 nan --synthetic', '--saxs_reweight: every THETA must be a positive finite number, got nan'),
    ('--saxs 16 --saxs_data curve.dat --saxs_reweight inf --synthetic', '--saxs_reweight: every THETA must be a positive finite number, got inf'),
    ('--saxs 16 --saxs_data curve.dat --saxs_reweight 10 -1 --synthetic', '--saxs_reweight: every THETA must be a positive finite number, got -1.0'),
    ('--saxs 16 --saxs_reweight 10 --synthetic', '--saxs_reweight needs --saxs_data: the curve the weighted mean is to agree with'),
    # each dependent flag without its parent
    ('--saxs_data curve.dat --synthetic', '--saxs_data needs --saxs: the curve is compared with the profile --saxs computes'),
    ('--saxs_hydration 1.0 0.5 --synthetic', '--saxs_hydration needs --saxs: it is the hydration shell and the contrast of the profile --saxs computes'),
    ('--saxs_hydration --synthetic', '--saxs_hydration needs --saxs: it is the hydration shell and the contrast of the profile --saxs computes'),
    ('--saxs_reweight 10 --synthetic', '--saxs_reweight needs --saxs: it reweights the structures against the profiles --saxs computes'),
    ('--compare_cluster 2.0 --synthetic', '--compare_cluster needs --compare'),
    ('--compare_cluster nan --synthetic', '--compare_cluster takes an RMSD cut-off in A, a positive number, got nan'),
    ('--pca_atoms all --synthetic', None),
    ('--cluster_atoms all --synthetic', None),
    # two faults: the order of the checks decides
    ('--stereo_check --relax -1 --synthetic --experiment bpd', '--stereo_check judges generated structures: --experiment bpd generates none'),
    ('--relax -1 --observables 0 --synthetic', '--relax takes a number of iterations >= 0, got -1'),
    ('--observables 0 --saxs 0 --synthetic', '--observables takes a number of test points per atom in 1 .. 1024, got 0'),
    ('--dssp --lddt --synthetic --experiment bpd', '--lddt scores generated structures against the true ones: --experiment bpd generates none'),
    ('--lddt --compare 0 --synthetic --experiment fmloss', '--compare takes the number of distance bins, 1 .. 256, got 0'),
    ('--pca 65 --cluster nan --synthetic', '--cluster takes an RMSD cut-off in A, a positive number, got nan'),
    ('--pr 0 --saxs_reweight 10 --synthetic', '--saxs_reweight needs --saxs: it reweights the structures against the profiles --saxs computes'),
    ('--saxs_hydration 1.0 --saxs_data curve.dat --synthetic', '--saxs_data needs --saxs: the curve is compared with the profile --saxs computes'),
    ('--geometry_check --stereo_check --data_process', '--geometry_check needs the topology of the structures: --data_process pickles carry none (use --pdb_files, --cg_pdb or --synthetic)'),
    ('--cluster 1.0 --geometry_check --synthetic --experiment bpd', '--geometry_check judges generated structures: --experiment bpd generates none'),
    ('--dssp --sampler ddim --model fm --synthetic --experiment bpd', '--dssp describes generated structures: --experiment bpd generates none'),
    ('--dssp --eta -1 --synthetic', '--eta must be >= 0, got -1.0'),
    ('--compare_cluster 2.0 --pca 0 --synthetic', '--pca takes the number of components, 1 .. 64, got 0'),
    ('--cg_pdb x.pdb --cg_xtc t.xtc --relax -1', '--relax takes a number of iterations >= 0, got -1'),
    ('--cg_pdb x.pdb --experiment bpd --dssp', "--cg_pdb needs --experiment latent: 'bpd' scores the latents of the input's atoms, and a CA-only input has none"),
    ('--saxs 0 --saxs_hydration 1.0 --synthetic', '--saxs takes a number of q values in 1 .. 512, got 0'),
    ('--saxs 16 --saxs_hydration 1.0 --saxs_reweight 10 --synthetic', '--saxs_hydration takes C1 and C2 or nothing (then both are fitted to --saxs_data), got 1 number(s)'),
    ('--relax -1 --synthetic --experiment bpd', '--relax takes a number of iterations >= 0, got -1'),
    ('--observables 0 --data_process', '--observables takes a number of test points per atom in 1 .. 1024, got 0'),
    ('--compare 257 --synthetic --experiment bpd', '--compare takes the number of distance bins, 1 .. 256, got 257'),
)


@pytest.mark.parametrize("line,refusal", CASES, ids=[line for line, _ in CASES])
def test_command_line_gets_the_recorded_answer(line, refusal):
    args = CLI.build_parser().parse_args(line.split())
    if refusal is None:
        assert CLI.check_args(args) is None
        return
    with pytest.raises(SystemExit) as e:
        CLI.check_args(args)
    assert e.value.code == refusal


def test_the_table_covers_every_flag_on_every_route_and_what_a_check_leaves_behind():
    lines = [line for line, _ in CASES]
    assert len(lines) == len(set(lines)) == 168
    routes = ("--synthetic", "--synthetic --experiment bpd", "--synthetic --experiment fmloss", "--data_process", "--cg_pdb x.pdb")
    given = {"--cluster": "--cluster 1.0", "--saxs_data": "--saxs 16 --saxs_data curve.dat", "--saxs_hydration": "--saxs 16 --saxs_hydration 1.0 0.5",
             "--saxs_reweight": "--saxs 16 --saxs_data curve.dat --saxs_reweight 10 1", "--compare_cluster": "--compare --compare_cluster 2.0",
             "--pca_atoms": "--pca --pca_atoms all", "--cluster_atoms": "--cluster 1.0 --cluster_atoms all"}
    flags = [row.flag for row in (CLI.RELAX,) + CLI.ANALYSES] + list(given)[1:]
    assert len(flags) == 17
    for flag in flags:
        for route in routes:
            assert f"{given.get(flag, flag)} {route}" in lines, (flag, route)
    # the normalisation the checks leave in the parser's namespace when nothing is on, and when everything is
    args = CLI.build_parser().parse_args(["--synthetic"])
    CLI.check_args(args)
    got = {k: getattr(args, k) for k in ("geometry_check", "stereo_check", "relax", "observables", "saxs", "saxs_hydration", "saxs_reweight",
                                          "pr", "cluster", "pca", "compare", "lddt", "dssp")}
    assert got == dict(geometry_check=False, stereo_check=False, relax=0, observables=0, saxs=0, saxs_hydration=None, saxs_reweight=(),
                       pr=0.0, cluster=0.0, pca=0, compare=0, lddt=False, dssp=False)
    assert [type(got[k]) for k in ("relax", "pr", "cluster", "pca")] == [int, float, float, int]
    assert not any(row.on(args) for row in (CLI.RELAX,) + CLI.ANALYSES)
    args = CLI.build_parser().parse_args("--cg_pdb x.pdb --relax --stereo_check --observables --saxs --saxs_hydration 1 0.5 --pr --cluster 2 --pca "
                                         "--compare --lddt --dssp".split())
    CLI.check_args(args)
    assert args.geometry_check is True and all(row.on(args) for row in (CLI.RELAX,) + CLI.ANALYSES)
    assert (args.relax, args.observables, args.saxs, args.saxs_hydration, args.pr, args.cluster, args.pca, args.compare) == \
        (200, 960, 51, (1.0, 0.5), 0.5, 2.0, 10, 50)
