"""GPU: metrics.lddt / codlad_lddt against tests/lddt_ref.py.

Every integer the device returns equals the float32 restatement exactly (the kernel's decisions are `fl32 < fl32` on values
made by one stated sequence of operations), every score is the float64 quotient of the device's own integers, and the
counts lie between the float64 counts with every cut moved in and out by the rounding margin of a float32 distance.
Shapes: the kernel's row block is 128 positions and its column tile 512, so 127 / 128 / 129 and 511 / 512 / 513 atoms."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from codlad_amd import _lib, metrics
from tests import lddt_ref as lr
from tests.test_buffer_discipline import hold

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INTS = ("atom_total", "atom_preserved", "residue_total", "residue_preserved", "swapped", "finite")
KEYS = INTS + ("residue", "global", "counts")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def host(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def same(a, b, keys=KEYS):
    return all(np.array_equal(a[k], b[k], equal_nan=a[k].dtype.kind == "f") for k in keys)


def check(out, models, refs, ref_index, res, sel=None, flip=None, **kw):
    """Every integer of `out` against the float32 restatement of each structure, and every score against the float64
    quotient of the device's own integers."""
    T = len(kw.get("thresholds", lr.THRESHOLDS))
    for s, f in enumerate(ref_index):
        want = lr.evaluate(models[s], refs[f], res, np.float32, sel=sel, flip=flip, **kw)
        for k in INTS:
            assert np.array_equal(out[k][s], want[k]), (s, k)
    fin = out["finite"]
    assert out["atom_total"].dtype == np.int32 and out["atom_preserved"].dtype == np.int32 and out["counts"].dtype == np.int64
    assert np.array_equal(out["counts"][fin, 0], out["atom_total"][fin].astype(np.int64).sum(1))
    assert np.array_equal(out["counts"][fin, 1:], out["atom_preserved"][fin].astype(np.int64).sum(1))
    assert out["atom_preserved"].shape[-1] == T and (out["counts"][~fin] == -1).all()
    assert np.array_equal(out["residue"][fin], lr.scores(out["residue_total"][fin], out["residue_preserved"][fin]), equal_nan=True)
    assert np.array_equal(out["global"][fin], lr.scores(out["counts"][fin, 0], out["counts"][fin, 1:]), equal_nan=True)
    assert np.isnan(out["residue"][~fin]).all() and np.isnan(out["global"][~fin]).all()


# ------------------------------------------------------------------------------------- restatement and float64 sandwich
@pytest.mark.parametrize("n,sigma", lr.CASES)
def test_integers_equal_the_restatement_and_lie_in_the_float64_sandwich(n, sigma):
    top, xyz = lr.chain(n)
    res = lr.residues(top)
    models = lr.noisy(xyz, sigma, seed=n, copies=2)
    out = host(metrics.lddt(dev(models), dev(xyz[None]), top))
    check(out, models, xyz[None], (0, 0), res, flip=lr.flips(top))
    plain = host(metrics.lddt(dev(models), dev(xyz[None]), top, symmetry=False))
    check(plain, models, xyz[None], (0, 0), res)
    assert not plain["swapped"].any() and np.array_equal(plain["atom_total"], out["atom_total"])
    for s in range(2):
        lo, hi, share = lr.sandwich(models[s], xyz, res)
        assert share <= lr.CAP
        assert (lo[0] <= plain["atom_total"][s]).all() and (plain["atom_total"][s] <= hi[0]).all()
        assert (lo[1] <= plain["atom_preserved"][s]).all() and (plain["atom_preserved"][s] <= hi[1]).all()
        ref64 = lr.evaluate(models[s], xyz, res, np.float64)
        print(f"n={n} sigma={sigma} s={s}: lDDT {plain['global'][s]:.6f} (float64 {ref64['score']:.6f}), with symmetry "
              f"{out['global'][s]:.6f}, {int(out['swapped'][s].sum())} residues swapped, undecided share {share:.1e}")


# ----------------------------------------------------------------------------------------------------- derived by hand
def lists(model, ref, res_ptr, **kw):
    return host(metrics.lddt_lists(dev(np.asarray(model, dtype=np.float32)[None]), dev(np.asarray(ref, dtype=np.float32)[None]),
                                   res_ptr, **kw))


def line(xs):
    x = np.zeros((len(xs), 3), dtype=np.float32)
    x[:, 0] = xs
    return x


def test_hand_derived_cases():
    model, ref, res_ptr, kept_sums, score = lr.toy()
    one = lists(ref, ref, res_ptr)
    assert one["global"].tolist() == [1.0] and one["residue"].tolist() == [[1.0, 1.0]] and one["atom_total"].tolist() == [[5, 1, 1, 1, 1, 1]]
    out = lists(model, ref, res_ptr)
    assert out["atom_preserved"][0].sum(1).tolist() == kept_sums and out["atom_preserved"][0, 0].tolist() == [1, 2, 3, 4]
    assert out["global"].tolist() == [score] and out["residue"].tolist() == [[0.5, 0.5]] and out["counts"].tolist() == [[10, 2, 4, 6, 8]]
    for shift, want in ((0.5, [0, 1, 1, 1]), (0.4375, [1, 1, 1, 1])):               # exactly 0.5 is not preserved at 0.5
        assert lists(line([0.0, 2.0 + shift]), line([0.0, 2.0]), [0, 1, 2])["atom_preserved"].tolist() == [[want, want]]
    below = float(np.nextafter(np.float32(15.0), np.float32(0.0)))
    for far, total in ((15.0, 0), (below, 1)):                                      # exactly 15 is not included
        got = lists(line([0.0, far]), line([0.0, far]), [0, 1, 2])
        assert got["atom_total"].tolist() == [[total, total]]
        assert np.isnan(got["global"]).all() if total == 0 else got["global"].tolist() == [1.0]
    single = lists(line([0.0, 1.0, 2.0]), line([0.0, 1.0, 2.0]), [0, 3])
    assert single["atom_total"].tolist() == [[0, 0, 0]] and np.isnan(single["residue"]).all() and np.isnan(single["global"]).all()
    assert single["finite"].tolist() == [True] and single["counts"].tolist() == [[0, 0, 0, 0, 0]]
    four = line([0.0, 1.0, 2.0, 3.0])
    assert lists(four, four, [0, 1, 2, 3, 4])["atom_total"].tolist() == [[3, 3, 3, 3]]
    assert lists(four, four, [0, 1, 2, 3, 4], seq_sep=2)["atom_total"].tolist() == [[2, 1, 1, 2]]


def test_a_rigid_motion_of_the_reference_scores_one():
    top, xyz = lr.chain(60)
    res = lr.residues(top)
    c, s = np.cos(0.7), np.sin(0.7)
    rot = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]]) @ np.array([[1.0, 0.0, 0.0], [0.0, 0.8, -0.6], [0.0, 0.6, 0.8]])
    moved = (xyz.astype(np.float64) @ rot.T + np.array([11.0, -7.0, 3.5])).astype(np.float32)
    out = host(metrics.lddt(dev(moved[None]), dev(xyz[None]), top))
    check(out, moved[None], xyz[None], (0,), res, flip=lr.flips(top))
    lo, hi, _share = lr.sandwich(moved, xyz, res)
    decided = np.ones(top.n_residues, dtype=bool)
    decided[res[(lo[0] != hi[0]) | (lo[1] != hi[1]).any(1)]] = False
    assert decided.sum() > top.n_residues // 2 and (out["residue"][0][decided] == 1.0).all() and not out["swapped"].any()


# ------------------------------------------------------------------------------------------------------------ symmetry
def exchanged(top, xyz, residues):
    """xyz [.., n, 3] with the coordinates of the symmetric atoms of `residues` exchanged, by the reference's table."""
    out = xyz.copy()
    for r in residues:
        for a, b in lr.flips(top)[r]:
            out[..., [a, b], :] = xyz[..., [b, a], :]
    return out


def test_exchanged_symmetric_groups_are_swapped_back_and_score_as_the_original():
    top, xyz = lr.chain(60)
    res = lr.residues(top)
    flip = lr.flips(top)
    assert {top.res_names[r] for r in flip} == set(lr.FLIPS)
    model = lr.noisy(xyz, 0.05, seed=5)[0]
    pick = sorted(flip)[::2]                                                        # every type, every other occurrence
    assert {top.res_names[r] for r in pick} == set(lr.FLIPS)
    both = np.stack([model, exchanged(top, model, pick)])
    out = host(metrics.lddt(dev(both), dev(xyz[None]), top))
    check(out, both, xyz[None], (0, 0), res, flip=flip)
    assert not out["swapped"][0].any() and np.nonzero(out["swapped"][1])[0].tolist() == pick
    assert same({k: v[0] for k, v in out.items() if k != "swapped"}, {k: v[1] for k, v in out.items() if k != "swapped"},
                [k for k in KEYS if k != "swapped"])
    off = host(metrics.lddt(dev(both), dev(xyz[None]), top, symmetry=False))
    check(off, both, xyz[None], (0, 0), res)
    assert not off["swapped"].any() and (off["residue"][1][pick] < out["residue"][1][pick]).all()
    others = np.setdiff1d(np.arange(top.n_residues), pick)
    assert np.array_equal(off["residue"][0], out["residue"][0]) and (off["residue"][1][others] <= out["residue"][1][others]).all()


def test_a_tie_keeps_the_naming_and_an_unselected_atom_ends_the_symmetry():
    top, xyz = lr.chain(60)
    res = lr.residues(top)
    flip = lr.flips(top)
    tie = next(r for r in sorted(flip) if top.res_names[r] == "ASP")
    model = lr.noisy(xyz, 0.05, seed=6)[0]
    (a, b), = flip[tie]
    model[a] = model[b] = 0.5 * (model[a] + model[b])                               # the exchange changes nothing: a tie
    model = exchanged(top, model, [r for r in flip if r != tie])
    out = host(metrics.lddt(dev(model[None]), dev(xyz[None]), top))
    check(out, model[None], xyz[None], (0,), res, flip=flip)
    assert np.nonzero(out["swapped"][0])[0].tolist() == sorted(r for r in flip if r != tie)
    phe = next(r for r in sorted(flip) if top.res_names[r] == "PHE")
    sel = np.array([i for i in range(top.n_atoms) if i != top.atom(phe, "CE1")])
    part = host(metrics.lddt(dev(model[None]), dev(xyz[None]), top, sel=sel))
    check(part, model[None], xyz[None], (0,), res, sel=sel, flip=lr.flips(top, set(sel.tolist())))
    assert not part["swapped"][0, phe] and part["swapped"][0].sum() == len(flip) - 2


# ------------------------------------------------------------------------------------------ the sizes of tile and block
def lattice_case(n, seed=0):
    ref = np.stack([lr.lattice(n), lr.lattice(n) + np.float32(0.25)])
    ref[1] = lr.noisy(ref[1], 0.4, seed + 1)[0]
    return lr.noisy(ref[0], 1.0, seed + 2, copies=3), ref, np.arange(n + 1)


@pytest.mark.parametrize("n", (2, 127, 128, 129, 511, 512, 513))
def test_lattices_at_the_row_block_and_the_column_tile(n):
    models, ref, res_ptr = lattice_case(n, seed=n)
    out = host(metrics.lddt_lists(dev(models), dev(ref), res_ptr, ref_index=(1, 0, 1)))
    assert out["atom_total"].shape == (3, n) and out["residue"].shape == (3, n)
    check(out, models, ref, (1, 0, 1), np.arange(n))
    assert n < 128 or out["counts"][:, 0].min() > 0
    alone = host(metrics.lddt_lists(dev(models[1:2]), dev(ref[:1]), res_ptr))       # S = 1, F = 1
    assert same({k: v[0] for k, v in alone.items()}, {k: v[1] for k, v in out.items()})


@pytest.mark.parametrize("thresholds", ((1.0,), (0.25, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 8.0), (4.0, 0.5, 2.0, 1.0, 1.0)))
def test_one_eight_and_unsorted_thresholds_and_a_frame_for_ten_members(thresholds):
    top, xyz = lr.chain(60)
    models = lr.noisy(xyz, 0.8, seed=len(thresholds), copies=10)
    out = host(metrics.lddt(dev(models), dev(xyz[None]), top, thresholds=thresholds, cutoff=10.0, seq_sep=3))
    assert out["atom_preserved"].shape == (10, top.n_atoms, len(thresholds))
    check(out, models, xyz[None], (0,) * 10, lr.residues(top), flip=lr.flips(top), thresholds=thresholds, cutoff=10.0, seq_sep=3)


# -------------------------------------------------------------------------------------------------------- independence
def test_a_structure_does_not_depend_on_the_call_it_is_in():
    top, xyz = lr.chain(60)
    models = lr.noisy(xyz, 0.8, seed=11, copies=5)
    refs = np.stack([xyz, lr.noisy(xyz, 0.2, seed=12)[0]])
    full = host(metrics.lddt(dev(models), dev(refs), top, ref_index=(0, 1, 0, 1, 1)))
    again = host(metrics.lddt(dev(models), dev(refs), top, ref_index=(0, 1, 0, 1, 1)))
    assert same(full, again)
    alone = host(metrics.lddt(dev(models[3:4]), dev(refs[1:2]), top))
    moved = host(metrics.lddt(dev(models[[3, 0]]), dev(refs), top, ref_index=(1, 0)))
    for other in (alone, moved):
        assert same({k: v[3] for k, v in full.items()}, {k: v[0] for k, v in other.items()})


def test_selection_order_and_unselected_atoms():
    top, xyz = lr.chain(60)
    res = lr.residues(top)
    models = lr.noisy(xyz, 0.8, seed=13, copies=2)
    rng = np.random.default_rng(14)
    sel = np.sort(rng.choice(top.n_atoms, top.n_atoms - 40, replace=False))
    perm = rng.permutation(sel.shape[0])
    a = host(metrics.lddt(dev(models), dev(xyz[None]), top, sel=sel))
    check(a, models, xyz[None], (0, 0), res, sel=sel, flip=lr.flips(top, set(sel.tolist())))
    b = host(metrics.lddt(dev(models), dev(xyz[None]), top, sel=sel[perm]))
    assert np.array_equal(b["atom_total"], a["atom_total"][:, perm]) and np.array_equal(b["atom_preserved"], a["atom_preserved"][:, perm])
    assert same(a, b, [k for k in KEYS if not k.startswith("atom_")])
    # a NaN in an atom that is not selected changes nothing, in the model or in the frame
    out_of = np.setdiff1d(np.arange(top.n_atoms), sel)
    bad_m, bad_r = models.copy(), xyz.copy()
    bad_m[0, out_of[0]], bad_r[out_of[-1], 1] = np.nan, np.inf
    assert same(a, host(metrics.lddt(dev(bad_m), dev(bad_r[None]), top, sel=sel)))
    ca = host(metrics.lddt(dev(models), dev(xyz[None]), top, sel=top.select("CA")))
    check(ca, models, xyz[None], (0, 0), res, sel=top.select("CA"), flip={})
    assert ca["atom_total"].shape == (2, 60) and not ca["swapped"].any()


# ---------------------------------------------------------------------------------------------------------- non-finite
def test_non_finite_structures_and_frames():
    top, xyz = lr.chain(60)
    res = lr.residues(top)
    models = lr.noisy(xyz, 0.8, seed=15, copies=5)
    refs = np.stack([xyz, lr.noisy(xyz, 0.2, seed=16)[0], xyz])
    index = (0, 1, 2, 1, 0)
    clean = host(metrics.lddt(dev(models), dev(refs), top, ref_index=index))
    bad_m = models.copy()
    bad_m[1, 7, 2], bad_m[3, top.n_atoms - 1, 0] = np.nan, -np.inf
    out = host(metrics.lddt(dev(bad_m), dev(refs), top, ref_index=index))
    check(out, bad_m, refs, index, res, flip=lr.flips(top))
    assert out["finite"].tolist() == [True, False, True, False, True]
    for k in ("atom_total", "atom_preserved", "residue_total", "residue_preserved", "counts"):
        assert (out[k][[1, 3]] == -1).all(), k
    assert np.isnan(out["residue"][[1, 3]]).all() and np.isnan(out["global"][[1, 3]]).all() and not out["swapped"][[1, 3]].any()
    keep = [0, 2, 4]
    assert same({k: v[keep] for k, v in out.items()}, {k: v[keep] for k, v in clean.items()})
    bad_r = refs.copy()
    bad_r[1, 100, 1] = np.nan                                                       # frame 1: models 1 and 3
    out = host(metrics.lddt(dev(models), dev(bad_r), top, ref_index=index))
    check(out, models, bad_r, index, res, flip=lr.flips(top))
    assert out["finite"].tolist() == [True, False, True, False, True]
    assert same({k: v[keep] for k, v in out.items()}, {k: v[keep] for k, v in clean.items()})


# -------------------------------------------------------------------------------------------------------------- limits
def abi_call(n=4, T=4, cutoff=15.0, thresholds=(0.5, 1.0, 2.0, 4.0, 8.0, 8.0, 8.0, 8.0, 8.0), seq_sep=1):
    """codlad_lddt on n single-atom residues through ctypes -> (return code, message, the outputs with their sentinel)."""
    import ctypes as C
    p = _lib.ptr
    i32 = lambda a: torch.tensor(a, dtype=torch.int32, device="cuda")                              # noqa: E731
    x = torch.zeros(1, n, 3, device="cuda")
    pos = torch.arange(n + 1, dtype=torch.int32, device="cuda")
    outs = dict(atom_total=torch.full((n,), -7, dtype=torch.int32, device="cuda"),
                atom_preserved=torch.full((n, 9), -7, dtype=torch.int32, device="cuda"),
                residue_total=torch.full((n,), -7, dtype=torch.int32, device="cuda"),
                residue_preserved=torch.full((n, 9), -7, dtype=torch.int32, device="cuda"),
                residue=torch.full((n,), -7.0, dtype=torch.float64, device="cuda"),
                counts=torch.full((10,), -7, dtype=torch.int64, device="cuda"),
                score=torch.full((1,), -7.0, dtype=torch.float64, device="cuda"),
                swapped=torch.full((n,), 0x5a, dtype=torch.uint8, device="cuda"),
                finite=torch.full((1,), 0x5a, dtype=torch.uint8, device="cuda"))
    thr = (C.c_float * len(thresholds))(*thresholds)
    rc = _lib.lib().codlad_lddt(p(x), 1, p(x), 1, p(i32([0])), n, None, 0, p(pos[:n].contiguous()), n, p(pos), p(pos[:n].contiguous()),
                                None, None, 0, C.c_float(cutoff), thr, T, seq_sep, *(p(t) for t in outs.values()), None,
                                _lib.stream_ptr(x.device))
    torch.cuda.synchronize()
    return rc, _lib.lib().codlad_last_error().decode(), outs


def test_one_past_each_declared_limit_is_refused():
    top, xyz = lr.chain(2)
    x = dev(xyz[None])
    with pytest.raises(ValueError, match="1 .. 8 thresholds .CODLAD_LDDT_MAX_THRESHOLDS."):
        metrics.lddt(x, x, top, thresholds=(0.5,) * 9)
    with pytest.raises(ValueError, match="cutoff must be positive finite"):
        metrics.lddt(x, x, top, cutoff=-15.0)
    with pytest.raises(ValueError, match="seq_sep must be an integer >= 1"):
        metrics.lddt(x, x, top, seq_sep=0)
    for bad in ((1,), (-1,), torch.tensor([1], device="cuda")):
        with pytest.raises(ValueError, match=r"ref_index has an entry outside \[0, 1\)"):
            metrics.lddt(x, x, top, ref_index=bad)
    with pytest.raises(ValueError, match="need a ref_index"):
        metrics.lddt(x.repeat(3, 1, 1), x.repeat(2, 1, 1), top)
    big = torch.zeros(1, _lib.LDDT_MAX_ATOMS + 1, 3, device="cuda")
    with pytest.raises(ValueError, match="at most 46340 atoms .CODLAD_LDDT_MAX_ATOMS."):
        metrics.lddt_lists(big, big, [0, 1, _lib.LDDT_MAX_ATOMS + 1])
    # the C entry point: a non-zero return, the message, and no output touched
    assert abi_call()[0] == 0
    for kw, msg in ((dict(T=9), "n_thresholds outside 1 .. CODLAD_LDDT_MAX_THRESHOLDS"), (dict(T=0), "n_thresholds outside"),
                    (dict(cutoff=-15.0), "cutoff is not a positive finite number"), (dict(cutoff=float("nan")), "cutoff is not"),
                    (dict(thresholds=(0.5, -1.0, 2.0, 4.0)), "a threshold is not a positive finite number"),
                    (dict(seq_sep=0), "seq_sep must be >= 1"), (dict(n=_lib.LDDT_MAX_ATOMS + 1), "CODLAD_LDDT_MAX_ATOMS")):
        rc, message, outs = abi_call(**kw)
        assert rc != 0 and "codlad_lddt: " in message and msg in message, (kw, message)
        assert all(bool((t == (0x5a if t.dtype == torch.uint8 else -7)).all()) for t in outs.values()), kw


def test_eight_thousand_atoms_on_sampled_rows():
    """n = 8192 single-atom residues, S = 2: 64 row blocks and 16 column tiles a structure; rows sampled from the first, the
    last and the blocks between against the restatement, the sums against the device's own rows."""
    n = 8192
    ref = lr.lattice(n, spacing=2.5)
    models = lr.noisy(ref, 0.7, seed=8192, copies=2)
    out = host(metrics.lddt_lists(dev(models), dev(ref[None]), np.arange(n + 1)))
    rows = np.unique(np.concatenate([np.arange(0, 130), np.arange(n - 130, n), np.random.default_rng(1).integers(0, n, 120)]))
    for s in range(2):
        total, kept = lr.counts(models[s], ref, np.arange(n), np.float32, rows=rows)
        assert np.array_equal(out["atom_total"][s, rows], total) and np.array_equal(out["atom_preserved"][s, rows], kept)
    assert np.array_equal(out["residue_total"], out["atom_total"]) and np.array_equal(out["residue_preserved"], out["atom_preserved"])
    assert np.array_equal(out["counts"][:, 0], out["atom_total"].astype(np.int64).sum(1)) and out["finite"].all()
    assert np.array_equal(out["global"], lr.scores(out["counts"][:, 0], out["counts"][:, 1:])) and (out["atom_total"] > 100).all()


def test_buffers_are_written_before_they_are_read():
    """tests/memcheck.py around lddt with symmetry, a selection and a structure that is not finite (its rows are written by
    the closing launch), and around lddt_lists at 513 positions: every output element is defined."""
    top, xyz = lr.chain(60)
    models = lr.noisy(xyz, 0.8, seed=21, copies=3)
    models[1, 5, 0] = np.nan
    sel = np.arange(top.n_atoms)[::-1][3:].copy()
    lat_m, lat_r, res_ptr = lattice_case(513, seed=3)

    def case(g):
        a = metrics.lddt(g(torch.from_numpy(models.copy()), "xyz"), g(torch.from_numpy(xyz[None].copy()), "ref"), top)
        top.__dict__.pop("_lddt_tables")                             # the next fill builds its own tables
        b = metrics.lddt(g(torch.from_numpy(models.copy()), "xyz_sel"), g(torch.from_numpy(xyz[None].copy()), "ref_sel"), top, sel=sel)
        c = metrics.lddt_lists(g(torch.from_numpy(lat_m.copy()), "xyz_lat"), g(torch.from_numpy(lat_r.copy()), "ref_lat"), res_ptr,
                               ref_index=(1, 0, 1))
        return {f"{n}_{k}": o[k] for n, o in (("all", a), ("sel", b), ("lat", c)) for k in KEYS}, []
    hold("lddt", case)


# ----------------------------------------------------------------------------------------------------------------- CLI
def _cli(cwd, *extra):
    cmd = [sys.executable, os.path.join(ROOT, "test.py"), "--synthetic", "--synthetic_weights", "--num_sampling_steps", "4",
           "--num_ensemble", "2"] + list(extra)
    res = subprocess.run(cmd, env=dict(os.environ, PYTHONPATH=ROOT), cwd=str(cwd), capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-1500:] + res.stderr[-3000:]
    files = {f: os.path.join(dp, f) for dp, _d, fs in os.walk(os.path.join(str(cwd), "logs")) for f in fs}
    return files, res.stdout


def test_cli_lddt_end_to_end(tmp_path):
    (tmp_path / "on").mkdir()
    (tmp_path / "off").mkdir()
    on, stdout = _cli(tmp_path / "on", "--lddt")
    off, stdout_off = _cli(tmp_path / "off")
    new = {f for f in on if f.endswith(("_lddt.npy", "_lddt_residue.npy"))}
    assert set(on) - set(off) == new and set(off) <= set(on) and len(new) == 2 * 4          # the four PED-shaped proteins
    for f in off:
        assert open(on[f], "rb").read() == open(off[f], "rb").read(), f                     # nothing else changes
    assert stdout.count("lddt synthetic_L") == 4 and "residues below 0.7" in stdout and "swapped symmetric residues" in stdout
    assert "lddt" not in stdout_off
    for L in (46, 87, 92, 129):
        xyz = np.load(on[f"synthetic_L{L}_xyz_recon.npy"])
        E, B = xyz.shape[:2]
        g, r = np.load(on[f"synthetic_L{L}_lddt.npy"]), np.load(on[f"synthetic_L{L}_lddt_residue.npy"])
        assert E == 2 and g.shape == (E * B,) and r.shape == (E * B, L) and g.dtype == r.dtype == np.float64
        assert ((g >= 0) & (g <= 1)).all() and ((r[~np.isnan(r)] >= 0) & (r[~np.isnan(r)] <= 1)).all()
    print("\n".join(line for line in stdout.splitlines() if line.startswith("lddt ")))
