"""Secondary structure (codlad_dssp_hbonds, codlad_dssp_assign, csrc/dssp_kernels.hip): the Kabsch-Sander hydrogen
bonds of every structure as bitmaps, the DSSP states read off them, and their propensity over the ensemble."""
import torch

from .. import _lib
from . import _inputs

DSSP_CODES = _lib.DSSP_CODES                     # " HBEGITS": the letter of code 0 .. 7; 255 (undefined) prints as '?'
DSSP_NAMES = ("loop", "H", "B", "E", "G", "I", "T", "S")
DSSP_MAX_RES = _lib.DSSP_MAX_RES


def dssp_tables(top):
    """(bb int32 [n_res, 4], res_kind uint8 [n_res]) of a dataset_builder.Topology, on the host: the atom indices of N, CA,
    C, O of every residue by atom name (-1: the residue lists none) and, per residue, bit 0 = PRO (no amide H), bit 1 = the
    residue starts a chain (residue 0, or chain_ids differs from the previous residue's: stereo_tables' neighbour rule).
    Built once and kept on the topology object."""
    def build():
        n_res = top.n_residues
        bb = torch.tensor([[top.atom(r, a) for a in ("N", "CA", "C", "O")] for r in range(n_res)],
                          dtype=torch.int32).reshape(n_res, 4)
        kind = torch.tensor([(_lib.DSSP_KIND_PRO if top.res_names[r] == "PRO" else 0) |
                             (_lib.DSSP_KIND_CHAIN_START if r == 0 or top.chain_ids[r - 1] != top.chain_ids[r] else 0)
                             for r in range(n_res)], dtype=torch.uint8)
        return bb, kind
    return _inputs.cached(top, "_dssp_tables", "host", build)


def _dssp_inputs(xyz, top, what):
    x = _inputs.structures(xyz, f"{what}: xyz", top.n_atoms)
    if not 1 <= top.n_residues <= DSSP_MAX_RES:
        raise ValueError(f"{what}: the topology has {top.n_residues} residues, the kernels take 1 .. {DSSP_MAX_RES}")
    return x, _inputs.cached(top, "_dssp_tables", str(x.device), lambda: tuple(t.to(x.device).contiguous() for t in dssp_tables(top)))


def hbonds(xyz, top):
    """Backbone hydrogen bonds of xyz [S, n_atoms, 3] (device), S structures of the topology `top` -> dict of device tensors
    (R = top.n_residues, W = ceil(R / 64); the rule is in include/codlad_hip.h):
      acc int64 [S, R, W]       bit j of row i (bit j % 64 of word j // 64): Hbond(i -> j), the C=O of i accepts the N-H of j
                                (E < -0.5 kcal/mol, Kabsch-Sander); the words are uint64 bit patterns held in int64
      don int64 [S, R, W]       bit j of row i: Hbond(j -> i); the transpose of acc
      geom uint8 [S, R]         bit 0: the link r -> r+1 is intact (same chain, C and N within 2.5 A); bit 1: bend (kappa > 70)
      kappa float32 [S, R]      the CA bend angle in degrees, NaN where undefined
      e_best float32 [S, R, 2], partner int32 [S, R, 2]
                                the lowest energy of the residue as acceptor ([..., 0]) and as donor ([..., 1]) and the partner
                                (ties: the lowest index); -1 and 0 where no pair is eligible
      finite bool [S]           False: a backbone coordinate is NaN or +-inf - bitmaps and geom 0, energies and kappa NaN,
                                partners -1
    Two launches, no host transfer; results are bit-identical from call to call and independent of the batch."""
    x, (bb, kind) = _dssp_inputs(xyz, top, "hbonds")
    return _hbonds_launch(x, bb, kind)[0]


def _hbonds_launch(x, bb, kind):
    dev = x.device
    S, R = x.shape[0], bb.shape[0]
    W = (R + 63) // 64
    acc = torch.empty(S, R, W, dtype=torch.int64, device=dev)
    don = torch.empty(S, R, W, dtype=torch.int64, device=dev)
    geom = torch.empty(S, R, dtype=torch.uint8, device=dev)
    kappa = torch.empty(S, R, dtype=torch.float32, device=dev)
    e_best = torch.empty(S, R, 2, dtype=torch.float32, device=dev)
    partner = torch.empty(S, R, 2, dtype=torch.int32, device=dev)
    finite = torch.empty(S, dtype=torch.uint8, device=dev)
    p = _lib.ptr
    rc = _lib.lib().codlad_dssp_hbonds(p(x), S, x.shape[1], p(bb), p(kind), R, p(acc), p(don), p(geom), p(kappa), p(e_best),
                                       p(partner), p(finite), _lib.stream_ptr(dev))
    _lib.check(rc, "codlad_dssp_hbonds")
    return dict(acc=acc, don=don, geom=geom, kappa=kappa, e_best=e_best, partner=partner, finite=finite.to(torch.bool)), finite


def dssp_assign(acc, don, geom, finite):
    """The pattern stage alone, on bitmaps in hbonds' layout (device; they need not come from hbonds) -> dict: ss uint8
    [S, R], bridge int32 [S, R, 2], counts int32 [S, 8]."""
    for t, what in ((acc, "acc"), (don, "don"), (geom, "geom"), (finite, "finite")):
        _inputs.need_cuda(t, what)
    S, R = geom.shape
    W = (R + 63) // 64
    if tuple(acc.shape) != (S, R, W) or tuple(don.shape) != (S, R, W) or tuple(finite.shape) != (S,) or S == 0 or R == 0:
        raise ValueError(f"dssp_assign: acc / don must be [S, R, ceil(R / 64)], geom [S, R], finite [S]; got "
                         f"{tuple(acc.shape)}, {tuple(don.shape)}, {tuple(geom.shape)}, {tuple(finite.shape)}")
    if acc.dtype != torch.int64 or don.dtype != torch.int64 or geom.dtype != torch.uint8:
        raise ValueError("dssp_assign: acc / don are int64 words, geom uint8")
    if R > DSSP_MAX_RES:
        raise ValueError(f"dssp_assign: {R} residues, the kernel takes 1 .. {DSSP_MAX_RES}")
    dev = geom.device
    fin = finite.to(torch.uint8).contiguous()
    ss = torch.empty(S, R, dtype=torch.uint8, device=dev)
    bridge = torch.empty(S, R, 2, dtype=torch.int32, device=dev)
    counts = torch.empty(S, 8, dtype=torch.int32, device=dev)
    p = _lib.ptr
    rc = _lib.lib().codlad_dssp_assign(p(acc.contiguous()), p(don.contiguous()), p(geom.contiguous()), p(fin), S, R, p(ss),
                                       p(bridge), p(counts), _lib.stream_ptr(dev))
    _lib.check(rc, "codlad_dssp_assign")
    return dict(ss=ss, bridge=bridge, counts=counts)


def ss_strings(ss):
    """ss uint8 [S, R] (any device) -> a list of S strings over DSSP_CODES, '?' for an undefined residue (one host copy)."""
    table = DSSP_CODES + "?" * (256 - len(DSSP_CODES))
    return ["".join(table[c] for c in row) for row in ss.detach().cpu().tolist()]


class _DsspResult(dict):
    """metrics.dssp's dict; `ss_string` is built (and the labels copied to the host) when it is first asked for."""

    def __missing__(self, key):
        if key != "ss_string":
            raise KeyError(key)
        self[key] = ss_strings(self["ss"])
        return self[key]


def dssp(xyz, top):
    """Secondary structure (DSSP: Kabsch & Sander 1983, classic priority H > B / E > G > I > T > S) of xyz [S, n_atoms, 3]
    (device), S structures of the topology `top` -> dict of device tensors:
      ss uint8 [S, R]             0 .. 7 = ' ', H, B, E, G, I, T, S (DSSP_CODES); 255 in a structure that is not finite
      ss_string                   a list of S strings over " HBEGITS", '?' for undefined; built on request only (out["ss_string"])
      bridge int32 [S, R, 2]      the lowest parallel and the lowest antiparallel bridge partner, -1 where there is none
      counts int32 [S, 8]         residues per code (-1: not finite), each also under its name: loop, H, B, E, G, I, T, S
      finite bool [S]
      acc, don, geom, kappa, e_best, partner: the first stage's tensors (hbonds)
    Three launches, no host transfer.  Differences from mkdssp: the full hydrogen-bond matrix is used (no truncation to a
    residue's two best partners), energies are not rounded to 0.001, there are no beta bulges and no sheet labels."""
    x, (bb, kind) = _dssp_inputs(xyz, top, "dssp")
    hb, finite = _hbonds_launch(x, bb, kind)
    out = _DsspResult(hb)
    out.update(dssp_assign(hb["acc"], hb["don"], hb["geom"], finite))
    out.update({k: out["counts"][:, c] for c, k in enumerate(DSSP_NAMES)})
    return out


def ss_propensity(ss):
    """ss uint8 [S, R] (device) -> float64 [R, 8] on the device: the share of the FINITE structures (those not labelled 255)
    that carry each code at each residue; NaN when no structure is finite."""
    _inputs.need_cuda(ss, "ss")
    if ss.dim() != 2 or ss.numel() == 0:
        raise ValueError(f"ss_propensity: ss must be a non-empty [S, R] tensor, got {tuple(ss.shape)}")
    codes = torch.arange(8, device=ss.device, dtype=ss.dtype)
    count = (ss[:, :, None] == codes).sum(dim=0).to(torch.float64)
    n_finite = (ss[:, 0] != _lib.DSSP_UNDEFINED).sum().to(torch.float64)
    # a tensor divisor: the correctly rounded quotient (a Python scalar would be turned into a multiplication by 1 / n)
    return count / n_finite
