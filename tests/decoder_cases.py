"""Cases and the comparison rule of the IC decoder's float64 parity test (tests/test_decoder_fp64_parity.py, GPU) and of
the CPU test that holds the cases to what they claim to be (tests/test_decoder_cases_host.py).

A case is a dict: vae_type ("N6": dec_heads_kernel<false>, "K3" / "K4": <true>), weights (key of `state_dict_of`), z_q
[M,3] (or [M,36] with latent_is_state), cg_z [M] int64, cg_xyz [M,3] float32, pairs [E,2] int64 and, per case, what was
aimed at.  `pairs` of the crafted cases is a DIRECTED list (receiver in column 0, sender in column 1, rows of both
orientations present), which Decoder.csr_from_pairs and oracle/vae_decode.py::directed take as given: in-degree and
distance are then set independently of the 21 A cutoff graph.

The rule (the project's, tests/test_fp64_parity.py): per residue and per channel, each channel scaled by its own
largest float64 value over the case,

    err_hip[residue, ch] <= c x max(e_ref[ch], FLOOR)

e_ref[ch] = the fp32 oracle's largest per-residue error against float64 in that channel, on the same inputs.
"""
import functools

import numpy as np
import torch

from codlad_amd import synth
from oracle import vae_decode as odec
from tests import cases
from tests import conditioning as cond

FLOOR = 1e-6
# c by CODLAD_OPT_DEC_EDGE_VARIANT: 1 keeps fp32 operands and the reference's order (as dec_init / dec_dense / dec_heads
# do), 0 (default) splits the filter's operands into 22 of 24 bits - the two bits f16x3 is granted in test_fp64_parity.py
C_VARIANT = {0: 16.0, 1: 4.0}
CUTOFF = 21.0
INDEGREES = (0, 1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 200)       # receivers 0..11 of the `indegree` case
ROWS_M = (2, 63, 64, 65, 129)
SWEEP_FLOOR, SWEEP_BELOW = "floor", "below"                         # coincident beads; the float32 just below 21
SWEEP_DISTANCES = ([SWEEP_FLOOR, 0.5, 1.0, 3.8, 10.5, 15.0] + [round(18.0 + 0.1 * i, 1) for i in range(30)]
                   + [20.99, 20.999, SWEEP_BELOW, 21.0, 21.5])
PERSISTENT_COPIES = 48
DATANAME = {"N6": "PED", "K3": "PDB", "K4": "Atlas"}


def _rng(seed):
    return np.random.Generator(np.random.PCG64(int(seed)))


# ---------------------------------------------------------------------------------------------------------------------
# weights and latents
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def state_dict_of(weights):
    """"N6" / "K3" / "K4": the synthetic VQ-VAE of that type; "realC2": the shipped C2 decoder weights behind a
    C2-scaled map_out (what test_ic_decode_and_xyz loads); "realC2_state": the same without map_out - the decoder
    takes a 36-wide latent as its state, as the C2 model does."""
    if weights in DATANAME:
        return synth.vqvae_state_dict(weights, DATANAME[weights], cases.VAE_SEED)
    sd = synth.vqvae_state_dict("N6", "PED", cases.VAE_SEED, c2_like_map_out=True)
    w = np.load(cases.npz_path("c2_decoder_weights"))
    for k in w.files:
        sd[k] = torch.from_numpy(w[k])
    if weights == "realC2_state":
        sd = {k: v for k, v in sd.items() if not k.startswith("map_out.")}
    elif weights != "realC2":
        raise KeyError(weights)
    return sd


def is_angle(case):
    return case["vae_type"] in ("K3", "K4")


def quantised_latent(vae_type, M, seed):
    """[M,3] rows of the codebook, as the VQ lookup hands them to the decoder (bit-exact on the device:
    test_vq_lookup_bit_exact)."""
    mean, std = synth.norm_stats(DATANAME[vae_type], vae_type)
    latent = synth.gaussian((M, 3), seed) * std + mean
    return odec.vq_lookup(latent, odec.codebook_of(state_dict_of(vae_type)))[0]


def _case(name, vae_type, z_q, cg_z, cg_xyz, pairs, weights=None, latent_is_state=False, **aim):
    M = cg_xyz.shape[0]
    cg_xyz = cg_xyz.float().contiguous()
    assert z_q.shape[0] == M and cg_z.shape == (M,) and pairs.dtype == torch.int64
    assert pairs.numel() == 0 or (0 <= int(pairs.min()) and int(pairs.max()) < M)      # the kernels trust the list
    assert 0 <= int(cg_z.min()) and int(cg_z.max()) < 25
    return dict(name=name, vae_type=vae_type, weights=weights or vae_type, z_q=z_q.float().contiguous(), cg_z=cg_z.long(),
                cg_xyz=cg_xyz, pairs=pairs.contiguous(), latent_is_state=latent_is_state, **aim)


def _is_directed_as_given(pairs):
    return bool((pairs[:, 0] > pairs[:, 1]).any()) and bool((pairs[:, 1] > pairs[:, 0]).any())


def kernel_distance(cg_xyz, directed_pairs):
    """The distance of every directed pair as the kernels form it, float32 operation by operation (the decoder's source
    is built without FMA contraction): sqrt(((rx rx + 1e-8) + (ry ry + 1e-8)) + (rz rz + 1e-8)), r = sender - receiver."""
    x = cg_xyz.float()
    r = x[directed_pairs[:, 1]] - x[directed_pairs[:, 0]]
    eps = torch.tensor(1e-8, dtype=torch.float32)
    sq = r * r + eps
    return torch.sqrt((sq[:, 0] + sq[:, 1]) + sq[:, 2])


def in_degrees(case):
    nb = odec.directed(case["pairs"]) if case["pairs"].numel() else case["pairs"]
    return torch.bincount(nb[:, 0], minlength=case["cg_xyz"].shape[0])


def _cutoff_pairs(xyz, nodes=None):
    """Directed (receiver, sender) rows of the true cutoff graph (synth.cg_nbr_list, both orientations), receiver-major;
    nodes: only these receivers."""
    und = synth.cg_nbr_list(xyz, CUTOFF)
    both = torch.cat([und, und.flip(1)])
    if nodes is not None:
        keep = torch.zeros(xyz.shape[0], dtype=torch.bool)
        keep[nodes] = True
        both = both[keep[both[:, 0]]]
    return both[torch.sort(both[:, 0], stable=True).indices]


# ---------------------------------------------------------------------------------------------------------------------
# the crafted cases
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def indegree_case(vae_type="N6"):
    """M = 260 beads, Gaussian with sigma 7 A (most pairs inside the cutoff, some outside), beads 100 and 101 coincident,
    residue types cycling through the 25 table rows.  Receivers 0..11 have exactly INDEGREES random senders each; every
    other residue has its true 21 A neighbourhood (in-degrees up to four 64-edge chunks)."""
    M, r = 260, _rng(811)
    xyz = torch.from_numpy((r.standard_normal((M, 3)) * 7.0).astype(np.float32))
    xyz[101] = xyz[100]
    rows = []
    for n, k in enumerate(INDEGREES):
        others = np.delete(np.arange(M), n)
        send = r.choice(others, size=k, replace=False)
        rows.append(torch.stack([torch.full((k,), n, dtype=torch.int64), torch.from_numpy(send).long()], 1))
    rows.append(_cutoff_pairs(xyz, nodes=torch.arange(len(INDEGREES), M)))
    pairs = torch.cat(rows)
    assert _is_directed_as_given(pairs)
    return _case(f"indegree_{vae_type}", vae_type, quantised_latent(vae_type, M, 821), torch.arange(M) % 25, xyz, pairs,
                 coincident=(100, 101))


@functools.lru_cache(maxsize=None)
def cutoff_sweep_case():
    """One sender on a ray from its receiver at each of SWEEP_DISTANCES; the edge is listed both ways, so receiver AND
    sender have in-degree 1 and one row of V is one edge's filter times one phi row.  Distances that must be hit
    exactly (coincident, the float32 below 21, 21.0, 21.5) lie along x from a receiver with x = 0, so that
    r = (d, 0, 0) holds exactly in float32 and the kernel's distance is d; the others point in seeded directions.
    48 more beads (Gaussian, sigma 7 A) with their true cutoff graph among themselves give every channel of V a scale
    from many-edge sums.  -> case with sweep = [(nominal, receiver, sender)]."""
    r = _rng(812)
    n = len(SWEEP_DISTANCES)
    below = float(np.nextafter(np.float32(CUTOFF), np.float32(0)))
    recv = (r.standard_normal((n, 3)) * 5.0).astype(np.float32)
    send = np.empty_like(recv)
    for k, d in enumerate(SWEEP_DISTANCES):
        if d == SWEEP_FLOOR:
            send[k] = recv[k]
        elif d in (SWEEP_BELOW, 21.0, 21.5):
            recv[k, 0] = 0.0
            send[k] = recv[k]
            send[k, 0] = np.float32(below if d == SWEEP_BELOW else d)
        else:
            u = r.standard_normal(3)
            send[k] = recv[k] + (np.float32(d) * (u / np.linalg.norm(u))).astype(np.float32)
    bg = (r.standard_normal((48, 3)) * 7.0).astype(np.float32)
    xyz = torch.from_numpy(np.concatenate([recv, send, bg]))
    M = xyz.shape[0]
    fwd = torch.stack([torch.arange(n), torch.arange(n) + n], 1)
    pairs = torch.cat([fwd, fwd.flip(1), _cutoff_pairs(xyz[2 * n:]) + 2 * n])
    assert _is_directed_as_given(pairs)
    sweep = [(d, k, k + n) for k, d in enumerate(SWEEP_DISTANCES)]
    return _case("cutoff_sweep", "N6", quantised_latent("N6", M, 822), (torch.arange(M) * 7) % 25, xyz, pairs, sweep=sweep)


def sweep_rows(case):
    """-> (rows int64 [2 n] of V with a single incoming edge, d float32 [2 n] their edge's distance as the kernel forms it,
    nominal list [2 n]): the receivers first, then the senders (the same edges the other way)."""
    nominal, recv, send = zip(*case["sweep"])
    recv, send = torch.tensor(recv), torch.tensor(send)
    rows = torch.cat([recv, send])
    d = kernel_distance(case["cg_xyz"], torch.stack([rows, torch.cat([send, recv])], 1))
    return rows, d, list(nominal) * 2


@functools.lru_cache(maxsize=None)
def rows_case(M):
    """The first M residues of one 129-residue chain with their true cutoff graph (the undirected j > i list)."""
    prot = synth.make_protein(129, 35, n_frames=1)
    xyz = torch.from_numpy(prot["xyz_full"])[0, 1:-1][:M]
    z = torch.from_numpy(prot["z_full"])[1:-1][:M]
    return _case(f"rows_{M}", "N6", quantised_latent("N6", M, 830 + M), z, xyz, synth.cg_nbr_list(xyz, CUTOFF))


@functools.lru_cache(maxsize=None)
def no_edges_case(M):
    """M residues of the same chain and an empty pair list: every message sum is zero."""
    c = rows_case(max(M, 2))
    return _case(f"no_edges_{M}", "N6", c["z_q"][:M], c["cg_z"][:M], c["cg_xyz"][:M], torch.zeros(0, 2, dtype=torch.int64))


@functools.lru_cache(maxsize=None)
def existing_case(name):
    """The shipped decoder geometries (cases.DECODER_CASES, realC2_L87_B2 with the shipped C2 weights) and
    realC2_state_L87_B2: the same weights and state without map_out, the 36-wide latent handed over as it is."""
    real = name.startswith("realC2")
    L, B, seed, vae_type = cases.DECODER_CASES["N6_L87_B2" if real else name]
    _prot, batch, latent, _dataname = cases.decoder_inputs(L, B, seed, vae_type)
    weights = name[:-len("_L87_B2")] if real else vae_type
    z_q = odec.vq_lookup(latent, odec.codebook_of(state_dict_of(vae_type)))[0].reshape(-1, 3)
    state = weights == "realC2_state"
    if state:
        sd = state_dict_of("realC2")
        z_q = torch.nn.functional.linear(z_q, sd["map_out.weight"], sd["map_out.bias"])
    return _case(name, vae_type, z_q, batch["CG_nxyz"][:, 0].long(), batch["CG_nxyz"][:, 1:], batch["CG_nbr_list"],
                 weights=weights, latent_is_state=state)


EXISTING = list(cases.DECODER_CASES) + ["realC2_L87_B2", "realC2_state_L87_B2"]


@functools.lru_cache(maxsize=None)
def persistent_parts():
    """The samples of the `persistent` job: PERSISTENT_COPIES copies of the N6_L87 structure and one N6_L46 structure, each
    with a latent of its own -> list of cases (one sample each)."""
    parts = []
    for k in range(PERSISTENT_COPIES + 1):
        L, _B, seed, vae_type = cases.DECODER_CASES["N6_L87_B2" if k < PERSISTENT_COPIES else "N6_L46_B3"]
        prot = synth.make_protein(L, seed, n_frames=1)
        xyz = torch.from_numpy(prot["xyz_full"])[0, 1:-1]
        z = torch.from_numpy(prot["z_full"])[1:-1]
        parts.append(_case(f"persistent_part{k}", vae_type, quantised_latent(vae_type, L, 900 + k), z, xyz,
                           synth.cg_nbr_list(xyz, CUTOFF)))
    return parts


def persistent_case():
    """All parts in one job (M = 48 x 87 + 46 = 4 222) -> (case, offsets of the parts)."""
    parts = persistent_parts()
    lens = [p["cg_xyz"].shape[0] for p in parts]
    offs = [0] + list(np.cumsum(lens))
    job = _case("persistent", "N6", torch.cat([p["z_q"] for p in parts]), torch.cat([p["cg_z"] for p in parts]),
                torch.cat([p["cg_xyz"] for p in parts]), torch.cat([p["pairs"] + o for p, o in zip(parts, offs)]))
    return job, [int(o) for o in offs]


# ---------------------------------------------------------------------------------------------------------------------
# references and the rule
# ---------------------------------------------------------------------------------------------------------------------
def oracle_run(case, dtype, phi_sub=None):
    """The oracle end to end from the case's z_q in `dtype` -> (ic [M,13,3], taps)."""
    sd = cond.to_dtype(state_dict_of(case["weights"]), dtype)
    taps = {}
    ic = odec.ic_decode(sd, case["z_q"], case["cg_z"], case["cg_xyz"], case["pairs"], angle=is_angle(case),
                        latent_is_state=case["latent_is_state"], taps=taps, phi_sub=phi_sub)
    assert ic.dtype == dtype and all(t.dtype == dtype for t in taps.values())
    return ic, taps


_refs = {}


def references(case):
    """{"ic": (fp32, float64) [M,39], "S": (fp32, float64) [M,40]} of the case, computed once and left unchanged."""
    if case["name"] not in _refs:
        (ic32, t32), (ic64, t64) = oracle_run(case, torch.float32), oracle_run(case, torch.float64)
        assert ic64.dtype == torch.float64 and t64["S4"].dtype == torch.float64 and ic32.dtype == torch.float32
        M = ic64.shape[0]
        _refs[case["name"]] = {"ic": (ic32.reshape(M, 39), ic64.reshape(M, 39)), "S": (t32["S4"], t64["S4"])}
    return _refs[case["name"]]


def message_references(case, phi, blk=3):
    """The message sum of block `blk` alone from the given phi [M,40] (a device's rows) -> (fp32, float64) [M,40]."""
    out = []
    for dtype in (torch.float32, torch.float64):
        sd = cond.to_dtype(state_dict_of(case["weights"]), dtype)
        out.append(odec.message_sum(sd, blk, phi, case["cg_xyz"], case["pairs"]))
        assert out[-1].dtype == dtype
    return tuple(out)


def table_channels(angle):
    """Channels of the flattened [13,3] output that are table rows: the bond lengths and, without the side-chain angle
    head, the ten side-chain angles."""
    ch = [3 * k for k in range(13)]
    if not angle:
        ch += [3 * k + 1 for k in range(3, 13)]
    return sorted(ch)


def e_ref_of(r32, r64):
    """[C]: the fp32 oracle's largest per-residue error against float64 per channel."""
    return cond.node_channel_error(r32, r64).amax(0)


def worst_ratio(got, r32, r64):
    """-> (ratio, residue, channel, err, e_ref): err / max(e_ref, FLOOR) where it is largest over every residue and
    channel of `got` [M,C]."""
    e_ref = e_ref_of(r32, r64)
    err = cond.node_channel_error(got, r64)
    ratio = err / e_ref.clamp_min(FLOOR)
    n, ch = divmod(int(ratio.argmax()), ratio.shape[1])
    return float(ratio.max()), n, ch, float(err[n, ch]), float(e_ref[ch])
