"""GPU: the denoiser on both sides of every size threshold of its dispatch, with every option at its shipped value.

enqueue_forward picks another kernel set per job size (launch_edge_now / launch_node in codlad_amd/csrc/denoiser_forward.hip,
node_kernel_h's placement in node_stream_kernel.hip); tests/large_job_cases.py builds, from short structures, a job on each
side of each threshold.  Three things are held here:

1. Every such job dispatches what its side of the threshold says - read from the dispatch record (codlad_dispatch_read:
   written by the code that picks the kernels and sizes the grids, not restated here) - and equals, bit for bit, `out` and
   the last decoder layer's h_V, the same members run in reference jobs of at most 1 024 nodes, whose record must show the
   small-job kernels (msg_wide_kernel / upd_wide_kernel, node_kernel_q, node_kernel_w) that tests/test_fp64_parity.py
   holds to float64 per edge and per node.  A sample's result does not depend on what shares its job (engine.py).
2. In the regimes no small job reaches - eight waves per node workgroup, XCD-chunked placement - three members of the
   big job's own result (the first, the last, one that lies across a chunk bound) are held to the float64 oracle by the
   rule and the bounds of tests/test_fp64_parity.py, imported from there.
3. `Denoiser.sample` over three steps, whole and as the two halves it deals by default, equals the reference jobs' loops.

Measured dispatch table, float64 ratios and durations: DESIGN.md section 2.
"""
import functools

import pytest
import torch

from codlad_amd import _lib, engine, synth
from codlad_amd.diffusion_and_flow.schedule import Tables, named_betas, space_timesteps
from tests import large_job_cases as lj
from tests import test_fp64_parity as fp

pytestmark = pytest.mark.gpu
DEV = fp.DEV
T_VALUE = 777
CASE_NAMES = list(lj.cases(256))                   # the names do not depend on the CU count; the targets do
FP64_CASES = ("nw4_max+1", "chunked_min")
LOOP_CASES = ("nw4_max+1", "two_halves")
SMALL = {"edge": "wide", "node_in": "w", "node_upd": "q"}       # what a reference job must dispatch in the split modes
F32 = {"edge": "f32", "node_in": "f32", "node_upd": "f32"}


def _cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


@functools.lru_cache(maxsize=None)
def _frames(L):
    return fp._frames(synth.make_protein(L, lj.STRUCT_SEED + L, n_frames=1))


_structures = {}


def structures_of(den, mode, lens):
    key = (mode, tuple(lens))
    if key not in _structures:
        fr = [_frames(L) for L in lens]
        _structures[key] = den.prepare_structures([f[0][0] for f in fr], [f[1] for f in fr])
    return _structures[key]


def _shows(rec, want):
    return all(rec[k] == v for k, v in want.items())


def _rec_text(rec):
    return (f"edge {rec['edge']} (grids msg {rec['grid_edge_msg']}, upd {rec['grid_edge_upd']}), input node kernel "
            f"{rec['node_in']} (grid {rec['grid_node_in']}{', chunked' if rec['chunked_in'] else ''}), node update "
            f"{rec['node_upd']} (grid {rec['grid_node_upd']}{', chunked' if rec['chunked_upd'] else ''})")


def _mismatch_report(what, lens, members, off, rec, differs, xcd_bounds):
    """differs: bool [n_nodes] on the CPU.  Names the first member that differs: its node range, where that lies
    relative to the node kernel's chunk bounds and the edge kernels' balanced ones, and its node-kernel workgroup."""
    n = int(off[-1])
    node = int(torch.nonzero(differs)[0])
    m = lj.member_of(off, node)
    a, b = int(off[m]), int(off[m + 1])
    chunk = lj.xcd_chunk_nodes(n)
    waves = {"h4": 4, "h8": 8}.get(rec["node_upd"])
    text = (f"{what}: {int(differs.sum())} of {n} nodes differ; first member {m} (L = {lens[members[m]]}, nodes {a}..{b - 1}), "
            f"first differing node {node}; node-kernel chunks of {chunk} nodes: the member starts {a % chunk} nodes after bound "
            f"{a // chunk} and ends {(-b) % chunk} nodes before bound {-(-b // chunk)}"
            f"{' - it lies across a chunk bound' if a // chunk != (b - 1) // chunk else ''}")
    if waves:
        c, wg, wave = lj.node_place(n, node, waves, rec["chunked_upd"])
        text += f"; node {node} belongs to workgroup {wg} of {rec['grid_node_upd']}, wave {wave}" + ("" if c is None else f", chunk {c}")
    return text + f"; edge-kernel chunk bounds {xcd_bounds}; record: {_rec_text(rec)}"


_big = {}


def big_run(name, mode):
    """One forward of the whole job of a case -> dict(lens, members, off, st, x (CPU), out, hV (device), rec, xcd_bounds).
    Computed once per (job, mode) and left unchanged."""
    cu = _cu()
    case = lj.cases(cu)[name]
    key = (case["target"], case["kind"], mode)
    if key not in _big:
        lens, members = lj.build_case(name, cu)
        off = lj.offsets(lens, members)
        den = fp.engine_of("eps", mode)
        st = structures_of(den, mode, lens)
        job = den.make_job(st, members)
        assert job.n_nodes == int(off[-1]) and int(job.ws.n_tiles) == lj.totals(lens, members)[1]
        x = synth.gaussian((job.n_nodes, 3), 4000 + case["target"] % 1000)
        out = den.forward(job, x.to(DEV), T_VALUE)
        rec = _lib.dispatch_read()
        _big[key] = dict(lens=lens, members=members, off=off, st=st, x=x, out=out, hV=job.hV.clone(), rec=rec,
                         xcd_bounds=job.xcd_bounds.cpu().tolist())
        del job
    return _big[key]


def reference_jobs(den, st, lens, members, mode):
    """The members in reference jobs of at most 1 024 nodes, one at a time -> (job, first node, end node); the caller
    checks by the dispatch record, after its launch on each, that it took the small-job kernels."""
    cu = _cu()
    off = lj.offsets(lens, members)
    groups = lj.ref_groups(lens, members, max_tiles=22 * cu, max_nodes=min(lj.REF_MAX_NODES, 64 * cu))
    for a, b in groups:
        yield den.make_job(st, members[a:b]), int(off[a]), int(off[b])


def _check_reference_record(mode, label):
    rec = _lib.dispatch_read()
    assert _shows(rec, F32 if mode == "f32" else SMALL), f"{label}: a reference job dispatched {_rec_text(rec)}"


@pytest.mark.parametrize("mode", fp.MODES)
@pytest.mark.parametrize("name", CASE_NAMES)
def test_both_sides_of_every_threshold(name, mode):
    cu = _cu()
    case = lj.cases(cu)[name]
    run = big_run(name, mode)
    lens, members, off, rec = run["lens"], run["members"], run["off"], run["rec"]
    n = int(off[-1])
    print(f"dispatch {name} {mode} ({cu} CUs; {n} nodes, {lj.totals(lens, members)[1]} edge tiles; {case['what']}): {_rec_text(rec)}")
    if mode == "f32":
        assert _shows(rec, F32), _rec_text(rec)
    else:
        for word, allowed in case["expect"].items():
            assert rec[word] in allowed, f"{name} {mode}: {word} is {rec[word]!r}, this side of the threshold says {allowed}: {_rec_text(rec)}"
    assert bool(torch.isfinite(run["out"]).all())
    den = fp.engine_of("eps", mode)
    x = run["x"].to(DEV)
    d_out = torch.zeros(n, dtype=torch.bool, device=DEV)
    d_hV = torch.zeros(n, dtype=torch.bool, device=DEV)
    n_refs = 0
    for rjob, a, b in reference_jobs(den, run["st"], lens, members, mode):
        n_refs += 1
        rout = den.forward(rjob, x[a:b], T_VALUE)
        _check_reference_record(mode, f"{name} {mode} nodes {a}..{b - 1}")
        d_out[a:b] = (rout != run["out"][a:b]).any(1)
        d_hV[a:b] = (rjob.hV != run["hV"][a:b]).any(1)
    print(f"dispatch {name} {mode}: compared with {n_refs} reference jobs")
    for what, d in (("h_V of the last decoder layer", d_hV), ("out", d_out)):
        assert not bool(d.any()), _mismatch_report(f"{name} {mode} {what}", lens, members, off, rec, d.cpu(), run["xcd_bounds"])


@pytest.mark.parametrize("mode", fp.MODES)
@pytest.mark.parametrize("name", FP64_CASES)
def test_new_regimes_against_float64(name, mode):
    """Members of the BIG job's own result against the float64 oracle: the member's spec alone, the device's h_E0 rows,
    neighbour lists and adaLN row for it (fp.device_run on the member as a job of its own), and out / h_V cut from the big
    job.  Rule and bounds: tests/test_fp64_parity.py."""
    run = big_run(name, mode)
    lens, members, off, rec = run["lens"], run["members"], run["off"], run["rec"]
    if mode != "f32":
        assert rec["node_upd"] in lj.H and (rec["chunked_upd"] or name != "chunked_min"), _rec_text(rec)
    straddlers = [(k, b, m) for k, b, m, s in lj.chunk_bound_members(off) if s]
    k, bound, m_bound = straddlers[0]
    picks = (("first", 0), ("last", len(members) - 1), (f"across chunk bound {k} (node {bound})", m_bound))
    den = fp.engine_of("eps", mode)
    for label, m in picks:
        a, b = int(off[m]), int(off[m + 1])
        xyz, z = _frames(lens[members[m]])
        spec = dict(kind="eps", xyz=xyz, z=[z], members=[0], x=run["x"][a:b], t=T_VALUE, x_sc=None)
        data = fp.device_run(den, spec)
        # the edge state the oracle is handed is the one the big job read: the structure's rows in the big job's set
        s0 = int(run["st"].offsets[members[m]])
        rows = engine.edge_rows(run["st"].h_E0[s0:s0 + b - a], split=den.split_edge_state).cpu()
        K = min(64, b - a)
        assert torch.equal(rows[:, :K], data["hE0"][0])
        assert torch.equal(run["st"].E_idx[s0:s0 + b - a, :K].cpu().long(), data["E_idx"][0])      # ... and its neighbour lists
        data["out"], data["hV"] = run["out"][a:b].cpu(), run["hV"][a:b].cpu()
        res = fp.ratios(spec, data)
        msg = "; ".join(f"{what}: err/e_ref {r:.2f} at node {nd} channel {c} (err {e:.2e}, e_ref {er:.2e})"
                        for what, (r, nd, c, e, er) in res.items())
        print(f"fp64 parity {name} {mode} member {m} ({label}; L = {b - a}, nodes {a}..{b - 1}) of the {int(off[-1])}-node job "
              f"[{rec['node_upd']}{', chunked' if rec['chunked_upd'] else ''}]: {msg}")
        for what, (r, _n, _c, _e, _er) in res.items():
            assert r <= fp.C_MODE[mode], f"{name} {mode} member {m} ({label}): {msg}"


@pytest.mark.parametrize("name", LOOP_CASES)
def test_sample_loops_whole_and_in_two_halves(name):
    """Denoiser.sample, T = 3, f16x3: the job whole on one stream and as the two halves `sample` deals by default, both
    against the reference jobs' loops on the same noise slices, x_0 and the last pred_xstart, bit for bit."""
    mode, T, cu = "f16x3", 3, _cu()
    lens, members = lj.build_case(name, cu)
    off = lj.offsets(lens, members)
    n = int(off[-1])
    den = fp.engine_of("eps", mode)
    st = structures_of(den, mode, lens)
    tb = Tables(named_betas("linear", 1000), space_timesteps(1000, str(T)))
    x_T, noise = synth.gaussian((n, 3), 5100 + n % 1000).to(DEV), synth.gaussian((T, n, 3), 5200 + n % 1000).to(DEV)
    job = den.make_job(st, members)
    assert den._n_streams(job, None) == 2
    got = {}
    for label, streams in (("whole", 1), ("two halves", None)):
        xs = torch.full((n, 3), float("nan"), device=DEV)           # the loop must write all of it
        x0 = den.sample(job, x_T, noise, tb, streams=streams, x_start_out=xs)
        rec = _lib.dispatch_read()
        got[label] = (x0, xs, rec)
        print(f"dispatch {name} {mode} sample {label} (the record of its last forward): {_rec_text(rec)}")
        assert bool(torch.isfinite(x0).all()) and bool(torch.isfinite(xs).all())
    halves = []
    for part, idx in job.parts(2):                   # each half's own record, from one forward of it
        den.forward(part, x_T[idx], T_VALUE)
        halves.append(_lib.dispatch_read())
        print(f"dispatch {name} {mode} half of {part.n_nodes} nodes: {_rec_text(halves[-1])}")
    whole_rec = got["whole"][2]
    for word, allowed in lj.cases(cu)[name]["expect"].items():
        assert whole_rec[word] in allowed, f"{name} sample whole: {word} is {whole_rec[word]!r}, not in {allowed}: {_rec_text(whole_rec)}"
    assert whole_rec["edge"] == "node", _rec_text(whole_rec)
    if name == "two_halves":
        assert [p.n_nodes for p, _i in job.parts(2)] == list(lj.HALVES)
        assert all(h["chunked_upd"] and h["chunked_in"] and h["node_upd"] in lj.H for h in halves)
    d = {(label, what): torch.zeros(n, dtype=torch.bool, device=DEV) for label in got for what in ("x_0", "pred_xstart")}
    n_refs = 0
    for rjob, a, b in reference_jobs(den, st, lens, members, mode):
        n_refs += 1
        rxs = torch.empty(b - a, 3, device=DEV)
        rx0 = den.sample(rjob, x_T[a:b], noise[:, a:b], tb, streams=1, x_start_out=rxs)
        _check_reference_record(mode, f"{name} sample nodes {a}..{b - 1}")
        for label, (x0, xs, _rec) in got.items():
            d[label, "x_0"][a:b] = (rx0 != x0[a:b]).any(1)
            d[label, "pred_xstart"][a:b] = (rxs != xs[a:b]).any(1)
    print(f"dispatch {name} {mode} sample: compared with {n_refs} reference loops")
    bounds = job.xcd_bounds.cpu().tolist()
    for (label, what), diff in d.items():
        assert not bool(diff.any()), _mismatch_report(f"{name} sample {label} {what}", lens, members, off, got[label][2],
                                                      diff.cpu(), bounds)
